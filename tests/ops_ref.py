"""Host-side fp64 references of the ops kernels (test infrastructure only).

ops_kernels.hip: Adam with its value / norm clip, DiagGauss, ZFilter apply and
column sums, moments, RewardFilter.  Every reference is plain torch in float64
and runs on the device of its inputs, so the two cases too large for the host
in a few seconds (Adam at 2^24 entries, DiagGauss at 4 M rows) evaluate it with
torch on the GPU.  tests/test_cpu_ops_ref.py checks each reference against
something independent (torch.optim.Adam in float64, oracle.ppo_ref on doubles)
and checks the conditions the GPU file relies on: that its inputs put rows on
both sides of every clamp and that the fp32 oracle itself stays inside each bar
on them.  tests/test_gpu_ops_edges.py takes its inputs, case tables and bars
from here.

Scalars of the C ABI are floats: a reference gets them as the library does,
rounded to fp32 (f32()), and computes in fp64 from there.  With beta2 = 0.999
that matters: 1 - fp32(0.999) is 1.3e-5 below 1e-3, and the bias correction
sees the same rounded beta2, so the quotient v / (1 - beta2^t) of the update
does not feel it.
"""
import math

import numpy as np
import torch

RTOL = 1e-5                 # fp32 elementwise outputs (helpers.max_rel_err, default floor)
NORM_RTOL = 2.5e-7          # one fp32 rounding (2^-24 = 6e-8) of an fp64 sum
SUM64_RTOL = 1e-9           # fp64 sums, relative to the sum of |terms|
U32 = 2.0 ** -24            # unit roundoff of fp32
CLAMP_LIK = 1e-5
LDS_CAP = 160 * 1024
WG = 256                    # threads of a workgroup (kWG)
NW = 4                      # its waves (kNW)


def f32(x):
    """a Python float as the C ABI passes it: rounded to fp32"""
    return float(np.float32(x))


# --------------------------------------------------------------------- Adam
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
ADAM_GRID_STRIDE_N = 2048 * 256 * 4 + 1029        # a second pass of the 2048-block grid + tail
ADAM_NT_N = (1 << 24) + 3                         # adam_kernel<3> + tail
# (weight_decay, max_norm, clip_value, eps)
ADAM_SETTINGS = ((0.0, 10.0, 0.0, 1e-8), (1e-3, 0.5, 0.0, 1e-8), (0.0, 0.0, 0.0, 1e-8),
                 (0.0, 0.0, 1.0, 1e-8), (1e-2, 0.0, 0.05, 1e-4), (0.0, 40.0, 0.0, 1e-4))
ADAM_STEPS = 6
ADAM_LR, ADAM_B1, ADAM_B2 = 3e-4, 0.9, 0.999
# float offsets of (p, g, m, v) from a 16-byte boundary
ADAM_ALIGN = {'aligned': (0, 0, 0, 0), 'g_offset': (0, 1, 0, 0), 'all_offset': (1, 2, 1, 2),
              'p_offset': (1, 0, 0, 0)}


def adam_params(n, seed, device='cpu'):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(n, generator=g).to(device)


def adam_grad(n, step, seed, device='cpu'):
    """gradient of step `step` (0-based): scale 3.0 / 0.01 alternating; in step 2
    every third entry is exactly 0"""
    g = torch.Generator().manual_seed(7919 * (step + 1) + seed)
    x = torch.randn(n, generator=g) * (0.01 if step % 2 else 3.0)
    if step == 2:
        x[::3] = 0.0
    return x.to(device)


def adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, max_norm, clip_value):
    """One step of smi_adam_clip (include/surreal_mi.h) in fp64: value clip, norm
    coefficient, weight decay, then m, v, p.  t = step count after this step.
    Returns p, m, v, the norm before the norm clip, and the effective gradient."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    if clip_value > 0:
        g = torch.clamp(g, -clip_value, clip_value)
    norm = torch.sqrt((g * g).sum())
    if max_norm > 0:
        g = g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    if wd != 0:
        g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    p = p - (lr / (1.0 - b1 ** t)) * (m / denom)
    return p, m, v, float(norm), g


# ---------------------------------------------------------------- DiagGauss
DG_ROW_A = tuple(range(1, 9))                  # diag_gauss_rows_kernel<A>
DG_LDS_A = (9, 12, 16, 31, 32)                 # diag_gauss_kernel
DG_ROWS = (1, 2, 255, 256, 257, 513)
DG_ROWS_2ND_PASS = (2 * 256 * 8192 + 5, 1)     # (rows, A): the row kernel's grid is 8192 x 2 rows
DG_LDS_2ND_PASS = (4096 * 256 + 300, 9)        # the LDS kernel's grid is 4096 tiles


def dg_sd_range(A):
    """std range of the policies: wide actions need a narrow one, or nearly
    every row's likelihood falls under the 1e-5 clamp"""
    return (0.2, 1.2) if A <= 9 else (0.15, 0.45)


def dg_spread(A):
    """per-row spread of the actions around the mean, in stds, ramped over the
    rows: narrow actions need a long ramp to reach the clamp at all"""
    return (0.25, 8.0 if A <= 2 else 4.0)


def dg_inputs(A, rows, seed=0):
    """actions [rows, A], prob0 and prob1 [rows, 2A] = [mean | std] (fp32, host)"""
    g = torch.Generator().manual_seed(100 * A + seed)
    lo, hi = dg_sd_range(A)

    def prob():
        return torch.cat([torch.rand(rows, A, generator=g) - 0.5,
                          lo + (hi - lo) * torch.rand(rows, A, generator=g)], 1)
    p0, p1 = prob(), prob()
    s = torch.linspace(*dg_spread(A), rows).view(-1, 1)
    a = p0[:, :A] + p0[:, A:] * s * torch.randn(rows, A, generator=g)
    return a, p0, p1


def dg_ref(a, p0, p1, A):
    """loglik, lik, kl, ent of smi_diag_gauss in fp64 (a / p1 may be None)"""
    out = {}
    m0, s0 = p0.double()[:, :A], p0.double()[:, A:]
    lsum = s0.log().sum(1)
    if a is not None:
        q = (((a.double() - m0) / s0) ** 2).sum(1)
        out['loglik'] = -0.5 * q - 0.5 * math.log(2.0 * math.pi) * A - lsum
        out['lik'] = torch.clamp(out['loglik'].exp(), min=CLAMP_LIK)
    if p1 is not None:
        m1, s1 = p1.double()[:, :A], p1.double()[:, A:]
        out['kl'] = ((s1 / s0).log().sum(1) +
                     ((s0 ** 2 + (m0 - m1) ** 2) / (2.0 * s1 ** 2)).sum(1) - 0.5 * A)
    out['ent'] = 0.5 * lsum + 0.5 * math.log(2.0 * math.pi * math.e) * A
    return out


def dg_row_floats(A):
    """floats of LDS per row staged by diag_gauss_kernel: actions | prob0 | prob1"""
    return (A | 1) + 2 * ((2 * A) | 1)


def dg_tile_rows(A):
    """the launcher's rows per tile: the largest multiple of 64 up to 256 whose
    tile fits the LDS of a CU; 0 = SMI_E_NOFIT"""
    R = WG
    while R > 0 and R * dg_row_floats(A) * 4 > LDS_CAP:
        R -= 64
    return R


def dg_first_rejected():
    A = 33
    while dg_tile_rows(A):
        A += 1
    return A


# ------------------------------------------------------------------ ZFilter
ZF_SHAPES = ((1, 1), (7, 3), (23, 17), (64, 42), (5, 64), (1, 1025))
ZF_EPS = 1e-5


def zf_state(dim, seed=0):
    """running buffers after one z_update of 200 rows with mean 0.25 .. 1.25 and
    std 2 (fp32): (sum, sumsq, count)"""
    g = torch.Generator().manual_seed(31 * dim + seed)
    x = torch.randn(200, dim, generator=g) * 2.0 + 0.25 + torch.rand(dim, generator=g)
    return x.sum(0), ZF_EPS + (x * x).sum(0), torch.tensor([ZF_EPS + 200.0])


def zf_input(rows, dim, seed=0):
    g = torch.Generator().manual_seed(17 * rows + dim + seed)
    return torch.randn(rows, dim, generator=g) * 6.0 + 0.5      # ~4 % beyond each of +-5 after the filter


def zf_apply_ref(x, rsum, rsumsq, count, eps):
    """ZFilter.forward (z_filter.py:59-79) in fp64 from the fp32 buffers; NaN
    propagates through both clamps, as in torch"""
    mean = rsum.double() / count.double()
    std = torch.clamp((rsumsq.double() / count.double() - mean ** 2).sqrt(), min=eps)
    return torch.clamp((x.double() - mean) / std, -5.0, 5.0)


# -------------------------------------------------------- column statistics
COL_SMALL = ((1, 64), (3, 65), (5, 200), (1000, 65))
COL_PARTIAL = ((700, 100), (257, 256), (256, 257), (300, 300), (65537, 1), (9000, 42))
COL_SMALL_MAX = 1 << 16           # rows * dim up to here: colstats_small_kernel


def col_input(rows, dim, stride, seed=0):
    """[rows, dim] view with row stride `stride` of data with mean 0.5 .. 1.5"""
    g = torch.Generator().manual_seed(rows + 3 * dim + seed)
    buf = torch.randn(rows, stride, generator=g) * 2.0 + 0.5 + torch.rand(stride, generator=g)
    return buf


def colsums_ref(x):
    x = x.double()
    return x.sum(0), (x * x).sum(0)


def col_chain(rows, dim, update):
    """(kernel form, L): L = the longest chain of sequential fp32 additions a
    column's sum goes through, in the kernels' order.

    small (rows * dim <= 65536): a thread adds the rows rl, rl + 4, ... of its
    column, ceil(rows / 4) additions; thread 0 of the column adds the 4 lane
    sums in order, 4 more.
    partial: gy workgroups along the rows take per = ceil(rows / gy) rows each;
    a thread adds every RP-th of them, ceil(per / RP) additions (the loop
    unrolled by 8 adds in the same order); RP lane sums are added in order;
    the finisher's thread p adds the partials p, p + 256, ..., ceil(gy / 256)
    additions, and block_sum_f (fp64 inside) rounds once to fp32.
    update mode adds the result to the running buffer: one more.  The square
    of an entry is rounded once before it is added: one more for the sums of
    squares (col_bound's `square`)."""
    if rows * dim <= COL_SMALL_MAX:
        return 'colstats_small_kernel', -(-rows // NW) + NW + (1 if update else 0)
    CB = min(dim, WG)
    RP = WG // CB
    gx = -(-dim // CB)
    gy = max(1, min(-(-rows // (8 * RP)), -(-2048 // gx)))
    per = -(-rows // gy)
    return 'colstats_finish_kernel', -(-per // RP) + RP + -(-gy // WG) + 1 + (1 if update else 0)


def col_bound(L, abs_terms, square=False):
    """L * 2^-24 * sum |terms| per column"""
    return (L + (1 if square else 0)) * U32 * abs_terms


# ------------------------------------------------------------------ moments
MOM_SIZES = (1, 65536, 65537, 65539, (1 << 21) + 5)
MOM_NP = (1, 256, 700)


def moments_ref(x):
    x = x.double()
    return float(x.sum()), float((x * x).sum()), float(x.abs().sum())


# ------------------------------------------------------------- RewardFilter
RF_SIZES = (1, 255, 256, 257, 5000)
RF_ROUNDS = 3
RF_SCALE = 0.5
RF_EPS = 1e-5


def rf_rewards(n, rnd, seed=0):
    g = torch.Generator().manual_seed(53 * n + rnd + seed)
    return torch.randn(n, generator=g) * 2.0 + 0.5


def rf_init(mode):
    """(running_sum, running_sumsq, count): the reference's initial filter where
    the rounds update it, the filter after 40 rewards of mean 0.3 and std 1.5
    where they only read it"""
    if mode & 2:
        return torch.tensor([0.0]), torch.tensor([0.0]), torch.tensor([RF_EPS])
    return torch.tensor([12.0]), torch.tensor([93.6]), torch.tensor([40.0 + RF_EPS])


def rf_forward_ref(x, rsum, rsumsq, count, eps):
    """RewardFilter.forward (reward_filter.py:44-56) in fp64 from the fp32 buffers"""
    mean = rsum.double() / count.double()
    std = torch.clamp((rsumsq.double() / count.double() - mean ** 2).sqrt(), min=eps)
    return torch.clamp((x.double() - mean) / std, -5.0, 5.0)


def rf_sums_ref(x):
    """{sum, sum of squares, n} of the (scaled) rewards in fp64, and sum |x|"""
    x = x.double()
    return torch.stack([x.sum(), (x * x).sum(), torch.tensor(float(x.numel()), dtype=torch.float64)]), \
        float(x.abs().sum())


def rf_update_ref(rsum, rsumsq, count, sums3):
    """RewardFilter.update (reward_filter.py:33-42) on fp32 buffers from fp64 sums:
    count += n, running_sum += sum, running_sumsq = sum of squares (the
    reference's `=`).  Returns fp64 values: the fp32 buffers are one (sumsq) or
    two (sum: the cast and the addition) fp32 roundings away."""
    return rsum.double() + sums3[0], sums3[1].clone().view(1), count.double() + sums3[2]


def rf_nan_sequence(rounds=6, n=64, seed=0):
    """rewards of mean 1.0 and std 0.3: with the `=` of the update the variance
    sumsq / count - mean^2 turns negative once count holds more than one batch"""
    g = torch.Generator().manual_seed(97 + seed)
    return [torch.randn(n, generator=g) * 0.3 + 1.0 for _ in range(rounds)]


# ---------------------------------------------------------- NaN faithfulness
def nan_filter_state(dim, neg_var=True):
    """running buffers written directly (count = 4, nothing depends on rounding):
    column 0: sumsq / count - mean^2 = -0.5 (std NaN: the column is NaN), or
              variance 1.5 with neg_var=False
    column 1: variance exactly 0 (std = eps)
    columns 2 ..: mean 0.5 * (c - 1), variance 1.5"""
    assert dim >= 4
    count = torch.tensor([4.0])
    mean = torch.tensor([1.0, 2.0] + [0.5 * (c - 1) for c in range(2, dim)])
    var = torch.tensor([-0.5 if neg_var else 1.5, 0.0] + [1.5] * (dim - 2))
    return mean * 4.0, (var + mean * mean) * 4.0, count


def nan_filter_input(rows, dim, seed=0):
    """column 1 holds its mean in every other row; column 2 holds NaN in every
    third row; column 3 holds +inf, -inf in rows 1, 2 mod 5"""
    g = torch.Generator().manual_seed(rows + dim + seed)
    x = torch.randn(rows, dim, generator=g) * 3.0 + 0.5
    x[::2, 1] = 2.0
    x[::3, 2] = float('nan')
    x[1::5, 3] = float('inf')
    x[2::5, 3] = float('-inf')
    return x


def same_nans(x, ref):
    x, ref = torch.as_tensor(x), torch.as_tensor(ref)
    return bool(torch.equal(torch.isnan(x), torch.isnan(ref)))


def max_rel_err_finite(x, ref, floor=None):
    """helpers.max_rel_err over the entries where the reference is not NaN"""
    from tests.helpers import max_rel_err
    x, ref = torch.as_tensor(x).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    keep = ~torch.isnan(ref)
    if not bool(keep.any()):
        return 0.0
    return max_rel_err(x[keep].numpy(), ref[keep].numpy(), floor=floor)


def rel_err_t(x, ref, floor=None):
    """helpers.max_rel_err in torch, on the device of `ref` (the large cases)"""
    x, ref = x.double().reshape(-1), ref.double().reshape(-1)
    if floor is None:
        floor = 1e-2 * max(1e-30, float(ref.abs().max()))
    return float(((x - ref).abs() / (ref.abs() + floor)).max())


def adam_scalars(setting):
    """the scalar arguments of smi_adam_clip for a row of ADAM_SETTINGS, as the
    library receives them"""
    wd, max_norm, clip_value, eps = setting
    return dict(lr=f32(ADAM_LR), b1=f32(ADAM_B1), b2=f32(ADAM_B2), eps=f32(eps), wd=f32(wd),
                max_norm=f32(max_norm), clip_value=f32(clip_value))
