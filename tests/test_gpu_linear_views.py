"""The three dense-layer calls and smi_linear_forward_cat on the operands the
learner hands them (surreal_amd/ddpg.py): leading dimensions wider than the
operand, bases 4-byte aligned only, outputs that are a column block of a wider
buffer, a ReLU output (exact zeros, its own leading dimension) or NULL as the
mask, act 0 / 1 / 2, b = NULL.

Every operand is a view into a NaN-filled buffer (tests/views.py; the checks
themselves are checked by tests/test_cpu_views.py).  Every case asserts

  * parity on the bar of the direct GEMM tests, _fp32_as_good_as_torch
    (fp32 torch on the CPU against the fp64 product, `mag` for the weight and
    bias gradients, slack 1e-6: every case has under 16384 rows),
  * every float outside an output's data region untouched, bit for bit,
  * no NaN in a data region (no padding reached a sum),
  * smi_last_launch() == the form pinned in the case table.

The pinned forms are derived from the dispatch rules of linear_kernels.hip
(launch_linear_fwd, gemm_launch, panel_ok, dx_smallk_launch, takes_t16,
takes_smallk_fwd) and linear_dw.hip / dw_plan.hpp (launch_linear_bwd_dw,
dwd_launch, dw_group_flush, dw_plan_rects); the comment of a case names the
branch it is there for.  A view is written 'wide4' (every operand) or
'x:off1,y:wide3' (those operands, the others tight).
"""
import math

import pytest
import torch

from surreal_amd import _lib as L
from tests import views as V
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# views beyond tests/views.py: an offset output at a 16-byte-multiple stride, and
# the action block of a wider weight, wc[:, c1:] (c1 floats in, ldw = c1 + A)
EXTRA = {'off1wide4': (4, 1), 'c1_20': (20, 20), 'c1_17': (17, 17)}

RED = 'gemm_splitk_reduce_kernel<%s>'
PF2, PF4, PF5 = ('gemm_panel_kernel<fwd,%d>' % c for c in (2, 4, 5))
PD2, PD4, PD5 = ('gemm_panel_kernel<dx,%d>' % c for c in (2, 4, 5))
TF, TD, TW = 'gemm_kernel<fwd>', 'gemm_kernel<dx>', 'gemm_kernel<dw>'
RTF, RTD, RTW = RED % TF, RED % TD, RED % TW
SK4, SK16 = 'gemm_smallk_fwd_kernel<4>', 'gemm_smallk_fwd_kernel<16>'
T16F, T16D = 'gemm_t16_kernel<fwd>', 'gemm_t16_kernel<dx>'
DWD, DWT16 = 'gemm_dwd_kernel', 'gemm_dwt16_kernel'
RDWD, DW128 = RED % DWD, RED % 'gemm_dw128_kernel'
COPY = 'copy_cols_kernel'
GROUP = 'group'                     # the grouped launch: its tile classes computed (_classes)


def setup_module(m):
    L.ensure_workspace(DEV)


def _last():
    return L.lib().smi_last_launch().decode()


def _lay(view, width):
    pad, off = EXTRA[view] if view in EXTRA else V.VIEWS[view]
    return width + pad, off


def _views(spec, names):
    if ':' not in spec:
        return {n: spec for n in names}
    vs = {n: 'tight' for n in names}
    for part in spec.split(','):
        n, v = part.split(':')
        assert n in vs, (n, names)
        vs[n] = v
    return vs


class _In:
    def __init__(self, t, view):
        self.t = t
        self.rows, self.cols = (1, t.numel()) if t.dim() == 1 else t.shape
        self.ld, self.off = _lay(view, self.cols)
        self.ptr, self.buf = V.make_in(t, self.ld, self.off, device=DEV)
        self.aligned = self.off % 4 == 0


class _Out:
    def __init__(self, rows, cols, view, init=None):
        self.rows, self.cols = rows, cols
        self.ld, self.off = _lay(view, cols)
        self.ptr, self.buf = V.make_out(rows, cols, self.ld, self.off, init=init, device=DEV)

    def check(self):
        return V.check_out(self.buf, self.rows, self.cols, self.ld, self.off)

    def untouched(self):
        """an output the call must not write at all."""
        V.assert_untouched(self.buf, self.rows, 0, self.ld, self.off)


ACT = {0: lambda z: z, 1: torch.relu, 2: torch.tanh}


def _weights(g, n, k):
    s = 1.0 / math.sqrt(k)
    return (2 * torch.rand(n, k, generator=g) - 1) * s, (2 * torch.rand(n, generator=g) - 1) * s


# ---------------------------------------------------------------- forward
# (rows, in, out, {view: form})
FWD_SHAPES = [
    # gemm_panel_kernel<fwd,2>: kept under wide4 (ldx = ldw = 72) and under a
    # misaligned / odd-ld output or bias (panel_ok looks at x and w only); dropped
    # to gemm_kernel<fwd> (4100 rows: no t16; K = 68 < 128: no split-K) by off1
    # on x, by off1 on w, by wide3 (ldx = 71)
    ((4100, 68, 24), {'tight': PF2, 'wide4': PF2, 'y:off1': PF2, 'y:wide3': PF2, 'b:off1': PF2,
                      'x:off1': TF, 'w:off1': TF, 'wide3': TF, 'off1wide3': TF}),
    # panel <fwd,4> / <fwd,5> kept under wide4 and an odd-ld misaligned output;
    # the tiled kernel with two column tiles (out 72) under off1wide3
    ((4100, 68, 60), {'wide4': PF4, 'y:off1': PF4, 'y:off1wide3': PF4, 'wide3': TF, 'off1wide3': TF,
                      'x:off1': TF, 'w:off1': TF}),
    ((4100, 68, 72), {'wide4': PF5, 'y:off1': PF5, 'wide3': TF, 'off1wide3': TF, 'x:off1': TF,
                      'w:off1': TF, 'x:wide3': TF}),
    # gemm_smallk_fwd_kernel (by shape alone): vec_out true (tight, wide4: ldy 40 / 44,
    # aligned) and false (wide3: ldy 43; off1 on y), ldx != K and ldw != K (wide views)
    ((2050, 12, 40), {'tight': SK4, 'wide4': SK4, 'wide3': SK4, 'off1wide3': SK4, 'x:off1': SK4,
                      'w:off1': SK4, 'y:off1': SK4}),
    # out 33: vec_out false at ldy 33 / 37, true at ldy 36 (y:wide3) with the
    # last 16-byte store of a row cut to one column
    ((2050, 16, 33), {'tight': SK4, 'wide4': SK4, 'wide3': SK4, 'off1wide3': SK4, 'x:off1': SK4,
                      'w:off1': SK4, 'y:off1': SK4, 'y:wide3': SK4}),
    ((4099, 64, 33), {'wide4': SK16, 'wide3': SK16, 'off1wide3': SK16, 'x:off1': SK16, 'w:off1': SK16,
                      'y:off1': SK16}),
    # gemm_t16_kernel<fwd>: a4 / b4 both (tight, wide4), a4 off (x:off1), b4 off
    # (w:off1), both off (wide3, off1wide3)
    ((300, 512, 40), {'tight': T16F, 'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F,
                      'w:off1': T16F, 'y:off1': T16F}),
    # gemm_splitk_reduce_kernel<gemm_kernel<fwd>> (K = 516 > 512, 5 tiles, 5 slabs)
    # writing through ldy > n; gemm_kernel's avec / bvec on (tight, wide4) and off
    ((300, 516, 40), {'tight': RTF, 'wide4': RTF, 'wide3': RTF, 'off1wide3': RTF, 'x:off1': RTF,
                      'w:off1': RTF, 'y:off1': RTF}),
    # the DDPG layer shapes of test_linear_ops_vs_torch: all t16 (< 256 tiles,
    # <= 4096 rows, K <= 512); K % 4 != 0 (17, 406, 5) never takes a4 / b4
    ((512, 17, 300), {'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F, 'w:off1': T16F,
                      'y:off1': T16F}),
    ((70, 406, 300), {'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F, 'w:off1': T16F,
                      'y:off1': T16F}),
    ((512, 300, 1), {'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F, 'w:off1': T16F,
                     'y:off1': T16F}),
    ((3, 5, 7), {'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F, 'w:off1': T16F,
                 'y:off1': T16F}),
    ((777, 100, 3), {'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F, 'w:off1': T16F,
                     'y:off1': T16F}),
    ((9, 256, 5), {'wide4': T16F, 'wide3': T16F, 'off1wide3': T16F, 'x:off1': T16F, 'w:off1': T16F,
                   'y:off1': T16F}),
]
# act cycles 0 / 1 / 2 and every fourth case passes b = NULL, per form, so each
# epilogue (panel, tiled, reducer, t16, small-K) sees all of them
FWD_CASES = []
_seen = {}
for (_r, _k, _n), _forms in FWD_SHAPES:
    for _spec, _form in _forms.items():
        _fam = _form.split(',')[0]
        _i = _seen.get(_fam, 0)
        _seen[_fam] = _i + 1
        FWD_CASES.append((_r, _k, _n, _i % 3, _i % 4 != 3, _spec, _form))


def test_forward_table_reaches_every_epilogue():
    """act 0, 1, 2 and b = NULL on the panel, tiled, reducer, t16 and small-K
    epilogues."""
    for fam in ('gemm_panel_kernel<fwd', TF, RTF, T16F, 'gemm_smallk_fwd_kernel'):
        mine = [c for c in FWD_CASES if c[6].startswith(fam)]
        assert {c[3] for c in mine} == {0, 1, 2}, fam
        assert any(not c[4] for c in mine) and any(c[4] for c in mine), fam


def _forward(rows, k, n, act, bias, spec, form, s_cols=0):
    vs = _views(spec, ('x', 'w', 'b', 'y', 's'))
    g = torch.Generator().manual_seed(rows * 131 + k * 17 + n + len(spec))
    x = torch.randn(rows, k, generator=g)
    W, b = _weights(g, n, k)
    xo, wo = _In(x, vs['x']), _In(W, vs['w'])
    bo = _In(b, vs['b']) if bias else None
    y = _Out(rows, n + s_cols, vs['y'])
    st = L.stream()
    if s_cols:
        s = torch.randn(rows, s_cols, generator=g)
        so = _In(s, vs['s'])
        L.call('smi_linear_forward_cat', xo.ptr, xo.ld, rows, k, wo.ptr, wo.ld, bo.ptr if bias else None,
               n, act, y.ptr, y.ld, so.ptr, so.ld, s_cols, st)
    else:
        L.call('smi_linear_forward', xo.ptr, xo.ld, rows, k, wo.ptr, wo.ld, bo.ptr if bias else None, n,
               act, y.ptr, y.ld, st)
    assert _last() == form
    got = y.check()                                  # canaries (the columns beyond included), no NaN
    z32 = x @ W.t() + (b if bias else 0)
    z64 = x.double() @ W.double().t() + (b.double() if bias else 0)
    _fp32_as_good_as_torch(got[:, :n], ACT[act](z32), ACT[act](z64))
    if s_cols:
        assert torch.equal(got[:, n:], s)


@pytest.mark.parametrize('rows,k,n,act,bias,spec,form', FWD_CASES,
                         ids=[f'{c[0]}x{c[1]}x{c[2]}-{c[5]}-act{c[3]}{"" if c[4] else "-nob"}'
                              for c in FWD_CASES])
def test_forward_views(rows, k, n, act, bias, spec, form):
    _forward(rows, k, n, act, bias, spec, form)


# (rows, in, out, s_cols, act, view, form)
CAT_CASES = [
    # the t16 path with xsrc (one launch), rows a multiple of 16 and not
    (512, 17, 400, 6, 1, 'tight', T16F),
    (512, 17, 400, 6, 2, 's:off1wide3,y:wide4', T16F),     # s strided and offset, ldy > out + s_cols
    (70, 406, 300, 6, 1, 'wide3', T16F),
    (70, 406, 300, 6, 0, 'off1wide3', T16F),
    # rows = 4096: the plain forward takes the panel (test below), the cat call t16
    (4096, 68, 24, 3, 1, 'tight', T16F),
    (4096, 68, 24, 3, 2, 's:wide3,y:off1wide3', T16F),
    # both fall-backs (forward, then copy_cols): after the small-K forward, after the panel
    (2050, 12, 40, 6, 1, 'tight', COPY),
    (2050, 12, 40, 6, 0, 's:off1wide3,y:wide3', COPY),
    (4100, 68, 24, 3, 1, 'wide4', COPY),
    (4100, 68, 24, 3, 2, 's:off1,y:off1wide3', COPY),
]


@pytest.mark.parametrize('rows,k,n,sc,act,spec,form', CAT_CASES,
                         ids=[f'{c[0]}x{c[1]}x{c[2]}+{c[3]}-{c[5]}' for c in CAT_CASES])
def test_forward_cat_views(rows, k, n, sc, act, spec, form):
    _forward(rows, k, n, act, True, spec, form, s_cols=sc)


def test_forward_4096_rows_plain_takes_the_panel():
    _forward(4096, 68, 24, 1, True, 'tight', PF2)


# --------------------------------------------------------- input gradient
# (rows, in, out, view, form with the mask, form with relu_mask = NULL)
V2, V4, V8, V8A = ('dx_smallk_kernel<%s>' % s for s in ('2,v4', '4,v4', '8,v4', '8,v4,a4'))
S1, S2, S4, S8 = ('dx_smallk_kernel<%d>' % k for k in (1, 2, 4, 8))
V1 = 'dx_smallk_kernel<1,v4>'
DX_STD = ('wide4', 'wide3', 'off1wide3', 'dy:off1', 'w:off1', 'dx:off1', 'mask:off1')


def _std(*forms):
    """the forms of one shape under DX_STD, in that order: the three joint views,
    then off1 on dy, on w, on the output, on the mask.  A pair is (with the mask,
    with relu_mask = NULL)."""
    assert len(forms) == len(DX_STD)
    return dict(zip(DX_STD, forms))


# (rows, in, out), {view: form, or (form with the mask, form with relu_mask = NULL)}
DX_SHAPES = [
    # dx_smallk_kernel by out_dim with every operand aligned: <1,v4> <2,v4> <4,v4>
    # <4,v4> <8,v4> <8,v4,a4>
    ((777, 100, 1), {'tight': V1}),
    ((777, 100, 2), {'tight': V2}),
    ((777, 100, 3), {'tight': V4}),
    ((777, 100, 4), {'tight': V4}),
    ((777, 100, 5), {'tight': V8}),
    ((777, 100, 8), {'tight': V8A}),
    # each v4 condition broken alone: in_dim % 4 (in 99), lddx % 4, dx base, ldw % 4,
    # w base, ldm % 4, mask base (the last two only with a mask); dy does not enter v4
    ((777, 99, 2), {'tight': S2, **_std(S2, S2, S2, S2, S2, S2, S2)}),
    ((777, 100, 2), {'dx:wide3': S2, 'w:wide3': S2, 'mask:wide3': (S2, V2),
                     **_std(V2, S2, S2, V2, S2, S2, (S2, V2))}),
    # each a4 condition broken alone: ldg % 4 (dy:wide3: ldg 11), dy base; v4 broken
    # under a4 falls to <8>; wide4: ldg 12, ldw / ldm / lddx 104
    ((777, 100, 8), {'dy:wide3': V8, **_std(V8A, S8, S8, V8, S8, S8, (S8, V8A))}),
    # the learner's dq call: ldg = 1, out_dim = 1 (512 x 300 x 1)
    ((512, 300, 1), {'tight': V1, **_std(V1, S1, S1, V1, S1, S1, (S1, V1))}),
    # in_dim % 4 != 0 (never v4); out_dim 3 and 5 (<4> and <8> with k past K masked)
    ((3, 5, 7), _std(S8, S8, S8, S8, S8, S8, S8)),
    ((777, 100, 3), _std(V4, S4, S4, V4, S4, S4, (S4, V4))),
    ((9, 256, 5), _std(V8, S8, S8, V8, S8, S8, (S8, V8))),
    # gemm_panel_kernel<dx,*> kept under wide4, under ldm != lddx and a misaligned
    # mask and output (panel_ok looks at dy and w only); the same shape dropped to
    # gemm_kernel<dx> (4100 rows: no t16; K = 20: no split-K) by off1 or wide3 on
    # dy or w
    ((4100, 96, 20), {'tight': PD2, 'dy:wide4,w:wide4,mask:off1wide3,dx:off1wide4': PD2,
                      'dy:wide3': TD, 'w:wide3': TD, **_std(PD2, TD, TD, TD, TD, PD2, PD2)}),
    ((4100, 116, 12), _std(PD4, TD, TD, TD, TD, PD4, PD4)),
    ((4100, 128, 20), {'mask:off1,dx:wide3': PD4, **_std(PD4, TD, TD, TD, TD, PD4, PD4)}),
    ((4100, 228, 12), _std(PD5, TD, TD, TD, TD, PD5, PD5)),
    ((4100, 240, 20), {'dx:off1wide3': PD5, **_std(PD5, TD, TD, TD, TD, PD5, PD5)}),
    # out_dim % 4 != 0 never takes the panel
    ((4099, 64, 33), _std(TD, TD, TD, TD, TD, TD, TD)),
    # gemm_t16_kernel<dx> with the mask (a4 on and off; b4 never: w is read along n)
    ((300, 40, 512), {'tight': T16D, **_std(T16D, T16D, T16D, T16D, T16D, T16D, T16D)}),
    ((512, 17, 300), _std(T16D, T16D, T16D, T16D, T16D, T16D, T16D)),
    ((70, 406, 300), _std(T16D, T16D, T16D, T16D, T16D, T16D, T16D)),
    # gemm_splitk_reduce_kernel<gemm_kernel<dx>> with the mask (K = 516: 5 slabs)
    ((300, 40, 516), {'tight': RTD, **_std(RTD, RTD, RTD, RTD, RTD, RTD, RTD)}),
    # a column block of a wider weight, as wc[:, c1:] is read: w offset by c1
    # floats, ldw = c1 + A, c1 a multiple of 4 and odd; on t16 and on dx_smallk
    ((512, 6, 300), {'w:c1_20': T16D, 'w:c1_17': T16D}),
    ((512, 4, 8), {'w:c1_20': V8A, 'w:c1_17': S8}),
]
DX_CASES = [(r, k, n, spec) + (f if isinstance(f, tuple) else (f, f))
            for (r, k, n), forms in DX_SHAPES for spec, f in forms.items()]


@pytest.mark.parametrize('rows,k,n,spec,form,form_nomask', DX_CASES,
                         ids=[f'{c[0]}x{c[1]}x{c[2]}-{c[3]}' for c in DX_CASES])
def test_backward_input_views(rows, k, n, spec, form, form_nomask):
    vs = _views(spec, ('dy', 'w', 'mask', 'dx'))
    g = torch.Generator().manual_seed(rows * 37 + k * 11 + n + len(spec))
    dy = torch.randn(rows, n, generator=g)
    W, _ = _weights(g, n, k)
    mask = V.relu_mask(rows, k, g)
    dyo, wo, mo = _In(dy, vs['dy']), _In(W, vs['w']), _In(mask, vs['mask'])
    r32, r64 = dy @ W, dy.double() @ W.double()
    keep = mask > 0
    st = L.stream()
    for masked, want in ((True, form), (False, form_nomask)):
        dx = _Out(rows, k, vs['dx'])
        L.call('smi_linear_backward_input', dyo.ptr, dyo.ld, rows, n, wo.ptr, wo.ld, k,
               mo.ptr if masked else None, mo.ld if masked else 0, dx.ptr, dx.ld, st)
        assert _last() == want
        got = dx.check()
        if masked:
            assert bool((got[~keep] == 0).all())            # exact and negative zeros do not pass
            _fp32_as_good_as_torch(got, r32 * keep, r64 * keep)
        else:
            _fp32_as_good_as_torch(got, r32, r64)


# -------------------------------------------------------- weight gradient
def _classes(out_dim, in_dim, db, a_al, b_al, ldg, ldx):
    """_classes of tests/test_gpu_dw_fit.py with the operands' alignment facts
    (dw_align, dw_group_add, dw_plan_rects): the tile classes of one grouped
    GEMM's rectangles in entry order."""
    M, N = out_dim, in_dim + (1 if db else 0)
    va = a_al and out_dim % 4 == 0 and ldg % 4 == 0 and out_dim >= 4
    vb = b_al and in_dim % 4 == 0 and in_dim >= 4 and ldx % 4 == 0
    Mf, Me, Nf, Ne = M // 64 * 64, M % 64, N // 64 * 64, N % 64
    mte = -(-Me // 16)
    if mte in (2, 3) and not a_al:
        mte = 4
    nte = 0
    if Ne:
        R = Ne - (1 if db else 0)
        nte = min(4, max(1, -(-R // 15)) if db else -(-R // 16))
        if nte in (2, 3) and not b_al:
            nte = 4
        if mte == 1 and not vb:
            nte = 4
    a = lambda mt: f'{mt}{("v" if va else "s") if mt == 4 else ""}'
    b = lambda nt: f'{nt}{("v" if vb else "s") if nt == 4 else ""}'
    out = []
    if Mf and Nf:
        out.append(f'{a(4)}x{b(4)}')
    if Me and Nf:
        out.append(f'{a(mte)}x{b(4)}')
    if Mf and Ne:
        out.append(f'{a(4)}x{b(nte)}')
    if Me and Ne:
        out.append(f'{a(mte)}x{b(nte)}')
    seen = []
    for c in out:
        if c not in seen:
            seen.append(c)
    return f'gemm_group_reduce_kernel<gemm_dwd_group_kernel<{",".join(seen)}>>'


def test_classes_agree_with_the_fitted_edge_tests():
    from tests.test_gpu_dw_fit import _classes as fit_classes, _form
    for o, i in ((8, 78), (72, 88), (90, 100), (108, 127), (128, 90), (400, 142)):
        for db in (0, 1):
            assert _classes(o, i, db, True, True, o, i) == _form(fit_classes(o, i, db))
    assert _classes(90, 100, 1, True, False, 90, 100) == _form(['4sx4s', '2x4s'])


DW_VIEWS = ('tight', 'wide4', 'wide3', 'off1wide3', 'dy:off1', 'x:off1', 'dw:off1', 'db:off1',
            'dw:off1wide3,db:off1')
# (rows, in, out, form of the call alone, form inside a begin / flush bracket),
# each under every view of DW_VIEWS: ldg / ldx in {w, w + 4, w + 3}, off1 on dy
# then x, lddw > in_dim, a misaligned dw and db.  Row-major weight gradients
# (both output sides <= 512) are dispatched by shape alone: gemm_dwd_kernel, with
# its split-K reducer above 128 rows; in a bracket gemm_dwt16_kernel up to 512
# rows, else the grouped launch (GROUP: its fitted-edge classes follow the
# operands' alignment and are computed by _classes).  An output side > 512 goes
# to the tiled engine: gemm_kernel<dw>, no split-K up to 128 rows.
DW_SHAPES = [
    (512, 17, 300, RDWD, DWT16),
    (70, 406, 300, DWD, DWT16),
    (512, 300, 1, RDWD, DWT16),                 # the learner's dq call: ldg = 1
    (3, 5, 7, DWD, DWT16),
    (9, 256, 5, DWD, DWT16),
    (4099, 64, 33, RDWD, GROUP),
    (777, 100, 3, RDWD, GROUP),
    (1100, 100, 90, RDWD, GROUP),
    (1100, 78, 72, RDWD, GROUP),
    (1100, 127, 108, RDWD, GROUP),
    (100, 20, 516, TW, TW),
]
# gemm_dw128_kernel (an output side > 512, >= 1024 rows, 16-byte operands) kept
# under wide4 and a misaligned dw / db; a misaligned or odd-stride dy or x sends
# the same shape to gemm_kernel<dw>.  Inside a bracket it launches at once.
DW128_VIEWS = {'tight': DW128, 'wide4': DW128, 'dw:off1': DW128, 'db:off1': DW128,
               'dw:off1wide3,db:off1': DW128, 'wide3': RTW, 'off1wide3': RTW, 'dy:off1': RTW,
               'x:off1': RTW, 'dy:wide3': RTW, 'x:wide3': RTW}
DW_CASES = [(r, k, n, grouped, spec, (f1, fg)[grouped])
            for r, k, n, f1, fg in DW_SHAPES for grouped in (0, 1) for spec in DW_VIEWS]
DW_CASES += [(1100, 96, 516, grouped, spec, f) for grouped in (0, 1) for spec, f in DW128_VIEWS.items()]
DW_CASES += [(1100, 127, 108, 1, 'dy:wide3,x:wide4', GROUP)]


@pytest.mark.parametrize('rows,k,n,grouped,spec,form', DW_CASES,
                         ids=[f'{c[0]}x{c[1]}x{c[2]}-{"grp" if c[3] else "one"}-{c[4]}' for c in DW_CASES])
def test_backward_weight_views(rows, k, n, grouped, spec, form):
    vs = _views(spec, ('dy', 'x', 'dw', 'db'))
    g = torch.Generator().manual_seed(rows * 29 + k * 7 + n + len(spec))
    x = torch.randn(rows, k, generator=g)
    dy = torch.randn(rows, n, generator=g)
    dyo, xo = _In(dy, vs['dy']), _In(x, vs['x'])
    w32, w64 = dy.t() @ x, dy.double().t() @ x.double()
    b32, b64 = dy.sum(0), dy.double().sum(0)
    mw = float((dy.abs().t() @ x.abs()).max())
    mb = float(dy.abs().sum(0).max())
    st = L.stream()
    for with_db in (1, 0):
        want = form
        if form == GROUP:
            want = _classes(n, k, with_db, dyo.aligned, xo.aligned, dyo.ld, xo.ld)
        for acc in (0, 1):                                  # plain, then accumulating into a known init
            w0 = torch.randn(n, k, generator=g) if acc else None
            b0 = torch.randn(n, generator=g) if acc else None
            dw = _Out(n, k, vs['dw'], init=w0)
            db = _Out(1, n, vs['db'], init=b0 if with_db else None)
            if grouped:
                L.call('smi_dw_group_begin')
            L.call('smi_linear_backward_weight', dyo.ptr, dyo.ld, rows, n, xo.ptr, xo.ld, k, dw.ptr,
                   dw.ld, db.ptr if with_db else None, acc, st)
            if grouped:
                L.call('smi_dw_group_flush', st)
            assert _last() == want
            got = dw.check()
            if acc:
                _fp32_as_good_as_torch(got, w0 + w32, w0.double() + w64, 1e-6, mw + float(w0.abs().max()))
            else:
                _fp32_as_good_as_torch(got, w32, w64, 1e-6, mw)
            if not with_db:
                db.untouched()
                continue
            gotb = db.check()[0]
            if acc:
                _fp32_as_good_as_torch(gotb, b0 + b32, b0.double() + b64, 1e-6, mb + float(b0.abs().max()))
            else:
                _fp32_as_good_as_torch(gotb, b32, b64, 1e-6, mb)


# ---------------------------------------------------------- argument checks
def test_leading_dims_smaller_than_the_width_are_refused():
    """ldg < out_dim, lddx < in_dim, ldm < in_dim (with a mask), ldx < in_dim:
    SMI_E_ARG and nothing written; the learner's calls (relu_mask = NULL with
    ldm = 0; ldg = 1 at out_dim = 1) still pass."""
    rows, k, n = 8, 12, 5
    g = torch.Generator().manual_seed(4)
    dy, x = torch.randn(rows, n, generator=g), torch.randn(rows, k, generator=g)
    W, _ = _weights(g, n, k)
    mask = V.relu_mask(rows, k, g)
    dyo, xo, wo, mo = (_In(t, 'tight') for t in (dy, x, W, mask))
    lib, st = L.lib(), L.stream()
    for ldg, ldm, lddx, masked in ((n - 1, k, k, True), (n, k - 1, k, True), (n, k, k - 1, True),
                                   (n, k, k - 1, False), (0, 0, k, False)):
        dx = _Out(rows, k, 'tight')
        rc = lib.smi_linear_backward_input(dyo.ptr, ldg, rows, n, wo.ptr, k, k, mo.ptr if masked else None,
                                           ldm, dx.ptr, lddx, st)
        assert rc == -1 and b'leading dims' in lib.smi_last_error()
        assert bool(torch.isnan(dx.buf).all())
    for ldg, ldx in ((n - 1, k), (n, k - 1), (0, k), (n, 0)):
        dw, db = _Out(n, k, 'tight'), _Out(1, n, 'tight')
        rc = lib.smi_linear_backward_weight(dyo.ptr, ldg, rows, n, xo.ptr, ldx, k, dw.ptr, k, db.ptr, 0, st)
        assert rc == -1 and b'leading dims' in lib.smi_last_error()
        assert bool(torch.isnan(dw.buf).all()) and bool(torch.isnan(db.buf).all())
    # the learner's calls
    dx = _Out(rows, k, 'tight')
    L.call('smi_linear_backward_input', dyo.ptr, n, rows, n, wo.ptr, k, k, None, 0, dx.ptr, k, st)
    _fp32_as_good_as_torch(dx.check(), dy @ W, dy.double() @ W.double())
    dq = torch.randn(rows, 1, generator=g)
    dqo, w1 = _In(dq, 'tight'), _In(W[:1].clone(), 'tight')
    dx = _Out(rows, k, 'tight')
    L.call('smi_linear_backward_input', dqo.ptr, 1, rows, 1, w1.ptr, k, k, mo.ptr, k, dx.ptr, k, st)
    keep = mask > 0
    _fp32_as_good_as_torch(dx.check(), (dq @ W[:1]) * keep, (dq.double() @ W[:1].double()) * keep)
    dw, db = _Out(1, k, 'tight'), _Out(1, 1, 'tight')
    L.call('smi_linear_backward_weight', dqo.ptr, 1, rows, 1, xo.ptr, k, k, dw.ptr, k, db.ptr, 0, st)
    _fp32_as_good_as_torch(dw.check(), dq.t() @ x, dq.double().t() @ x.double(), 1e-6,
                           float((dq.abs().t() @ x.abs()).max()))
    _fp32_as_good_as_torch(db.check()[0], dq.sum(0), dq.double().sum(0), 1e-6, float(dq.abs().sum()))
