"""Direct tests of dqn_kernels.hip through the C ABI (smi_dqn_td, smi_dqn_greedy).

References are fp64 numpy over the same fp32 inputs.  Operands are views with
poison and canaries (tests/views.py).  Scores are multiples of 1/8, distinct
within a row, so no fp32 rounding can change an arg-max; designated rows hold
exact ties (equal bit patterns at two or three positions, position 0 and the
last included): identical inputs go through identical operations, the ties stay
ties under the dueling combination, and the chosen index must be the first.

Numeric bars (u = 2^-24, one fp32 rounding; first order, times 1 + 2^-10 for the
higher orders, plus 1e-30), from the expressions the kernel evaluates:
  s    = a_0 + ... + a_{A-1}, left to right: A - 1 roundings of partial sums that
         are integers / 8 below 2^24 / 8, i.e. EXACT here
  m    = s / A                      e_m  = u |m|
  q_j  = (a_j - m) + v              e_q  = e_m + u |a_j - m| + u |q_j|     (0 without dueling)
  y    = r + gamma ((1 - d) q')     e_y  = gamma e_q' + u |gamma q'| + u |y|   (1 - d, (1 - d) q' exact)
  td   = q_a - y                    e_td = e_q(a) + e_y + u |td|
  l    = 0.5 td^2 | |td| - 0.5      e_l  = (min(|td|, 1) + e_td) e_td + 2 u l  (slope <= min(|td|, 1)
                                           on either branch; C1 at |td| = 1, so no row is excluded)
  g    = (w clamp(td)) / B          e_g  = w e_td / B + 2 u |g|
  dadv = g ([j == a] - 1/A)         e_d  = e_g |c| + |g| (u / A + u |c|) + u |dadv|, c = [j == a] - 1/A
         g [j == a] without dueling: e_g at j == a, exactly 0 elsewhere
  stats: fp64 sums of the fp32 terms, one final rounding:
         loss  mean(w e_l + u w l) + u loss;   td  mean(e_td) + u mean|td|
Exact: j* (through y_out where the target scores of a row are distinct, and
through smi_dqn_greedy), the zero pattern of dadv without dueling, dval (and
dadv[a] without dueling) = fl(fl(w * clamp(td_out)) / B) from the kernel's own
td_out, w = NULL against w = 1, y == r on terminal rows, the canaries.
"""
import ctypes

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from tests import views as V

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
HI = 1 + 2.0 ** -10
E_ARG = -1
GAMMA = 0.99
BS, AS = (1, 255, 257, 1025), (1, 2, 3, 18)
FORMS = ((1, 1), (1, 0), (0, 1), (0, 0))
VIEW_NAMES = ('tight', 'wide3', 'wide4', 'off1', 'off1wide3')


def _st():
    return L.stream()


def _last():
    return L.lib().smi_last_launch().decode()


def _err():
    return L.lib().smi_last_error().decode()


def _scores(B, A, rs, ties):
    """[B][A] multiples of 1/8 in [-5, 5], distinct within a row; with `ties`
    rows i % 7 == 0 / 3 / 5 get their maximum at (0, last) / (0, A // 2, last) /
    (1, last).  Returns (scores, expected first arg-max)."""
    x = np.stack([rs.permutation(81)[:A] - 40 for _ in range(B)]).astype(np.float64) / 8
    if ties and A >= 2:
        for i in range(B):
            pos = {0: (0, A - 1), 3: (0, A // 2, A - 1), 5: (1, A - 1)}.get(i % 7)
            if pos is None or (A < 3 and i % 7 != 0):
                continue
            x[i, list(pos)] = 5.125
    return x.astype(np.float32), x.argmax(1)


def _col(x, stride, off):
    """x [n] as column 0 of a poisoned [n][stride] buffer"""
    return V.make_in(torch.as_tensor(x, dtype=torch.float32).view(-1, 1), stride, off, DEV)


def _exact_mean_rows(adv, act, rows):
    """make the row sums of `rows` multiples of A / 8 (the mean, and with it
    every q_j, exact) by moving one non-action, non-extreme entry"""
    A = adv.shape[1]
    for i in rows:
        if A < 3:
            continue
        j = next(k for k in range(A) if k != act[i] and k != adv[i].argmax())
        for cand in np.arange(-80, 81) / 8.0 - 20:          # far below every other score
            t = adv[i].astype(np.float64).copy()
            t[j] = cand
            if round(t.sum() * 8) % A == 0:
                adv[i, j] = cand
                break


def _case(B, A, dueling, double_q, seed):
    rs = np.random.RandomState(seed)
    adv, _ = _scores(B, A, rs, ties=False)
    adv_n, _ = _scores(B, A, rs, ties=bool(double_q))
    adv_t, _ = _scores(B, A, rs, ties=not double_q)
    val, val_n, val_t = (rs.randint(-24, 25, size=B).astype(np.float32) / 8 for _ in range(3))
    act = rs.randint(0, A, size=B)
    rew = rs.randn(B).astype(np.float32) * 2
    done = (rs.rand(B) < 0.25).astype(np.float32)
    w = (0.25 + rs.randint(0, 7, size=B) / 8).astype(np.float32)
    # rows with td exactly +-1 and just on either side: terminal, exact q(s)[a]
    edge = [i for i in range(min(B, 40)) if i % 5 == 1][:4]
    _exact_mean_rows(adv, act, edge)
    for i, d in zip(edge, (1.0, -1.0, 1.125, 0.875)):
        a64 = adv[i].astype(np.float64)
        q = (a64[act[i]] - a64.sum() / A) + val[i] if dueling else a64[act[i]]
        done[i], rew[i] = 1.0, np.float32(q - d)            # A < 3: s / A is exact anyway
    return dict(adv=adv, adv_n=adv_n, adv_t=adv_t, val=val, val_n=val_n, val_t=val_t, act=act,
                rew=rew, done=done, w=w, edge=edge)


def _reference(c, A, dueling, double_q, weighted):
    """fp64 values and the first-order error bounds of the module docstring"""
    f = lambda k: c[k].astype(np.float64)                              # noqa: E731
    B = c['adv'].shape[0]
    g32 = float(np.float32(GAMMA))
    rows = np.arange(B)

    def q_of(a, v):
        if not dueling:
            return a, np.zeros_like(a)
        m = a.sum(1, keepdims=True) / A
        q = (a - m) + v[:, None]
        return q, U * np.abs(m) + U * np.abs(a - m) + U * np.abs(q)
    q, eq = q_of(f('adv'), f('val'))
    qt, eqt = q_of(f('adv_t'), f('val_t'))
    scan = q_of(f('adv_n'), f('val_n'))[0] if double_q else qt
    js = scan.argmax(1)                                                # first maximum
    qn, eqn = qt[rows, js], eqt[rows, js]
    live = 1 - f('done')
    y = f('rew') + g32 * (live * qn)
    ey = g32 * live * eqn + U * np.abs(g32 * live * qn) + U * np.abs(y)
    td = q[rows, c['act']] - y
    etd = eq[rows, c['act']] + ey + U * np.abs(td)
    ab = np.abs(td)
    l = np.where(ab < 1, 0.5 * td * td, ab - 0.5)
    el = (np.minimum(ab, 1) + etd) * etd + 2 * U * l
    w = f('w') if weighted else np.ones(B)
    g = w * np.clip(td, -1, 1) / B
    eg = w * etd / B + 2 * U * np.abs(g)
    onehot = np.zeros((B, A))
    onehot[rows, c['act']] = 1
    if dueling:
        cf = onehot - 1.0 / A
        dadv = g[:, None] * cf
        ed = eg[:, None] * np.abs(cf) + np.abs(g)[:, None] * (U / A + U * np.abs(cf)) + U * np.abs(dadv)
    else:
        dadv, ed = g[:, None] * onehot, eg[:, None] * onehot
    loss, mtd = (w * l).mean(), ab.mean()
    return dict(js=js, qt=qt, y=y, ey=ey, td=td, etd=etd, g=g, eg=eg, dadv=dadv, ed=ed, loss=loss,
                eloss=(w * el + U * w * l).mean() + U * loss, mtd=mtd, emtd=etd.mean() + U * mtd)


def _run(c, A, dueling, double_q, weighted, view, y_out=True):
    """one smi_dqn_td call over view operands; returns the checked outputs"""
    B = c['adv'].shape[0]
    pad, off = V.VIEWS[view]
    ld = A + pad
    keep = []

    def mat(x):
        p, b = V.make_in(torch.from_numpy(x), ld, off, DEV)
        keep.append(b)
        return p

    def col(x, stride):
        p, b = _col(x, stride, off)
        keep.append(b)
        return p
    dp, dbuf = V.make_out(B, A, ld, off, device=DEV)
    outs = {k: V.make_out(1, n, n, off, device=DEV) for k, n in
            (('dval', B), ('td', B), ('y', B), ('stats', 2))}
    L.call('smi_dqn_td', mat(c['adv']), ld, mat(c['adv_n']) if double_q else None, ld,
           mat(c['adv_t']), ld,
           col(c['val'], 1 + pad) if dueling else None, 1 + pad,
           col(c['val_n'], 2) if dueling and double_q else None, 2,
           col(c['val_t'], 3) if dueling else None, 3,
           col(c['act'], 1 + pad), 1 + pad, col(c['rew'], 2 + pad), 2 + pad, col(c['done'], 3), 3,
           col(c['w'], 1) if weighted else None, B, A, GAMMA, dueling, double_q, dp, ld,
           outs['dval'][0] if dueling else None, outs['td'][0], outs['y'][0] if y_out else None,
           outs['stats'][0], _st())
    assert _last() == f'dqn_td_kernel<{dueling},{double_q}>'
    res = {'dadv': V.check_out(dbuf, B, A, ld, off)}
    for k, n in (('dval', B), ('td', B), ('y', B), ('stats', 2)):
        buf = outs[k][1]
        if (k == 'dval' and not dueling) or (k == 'y' and not y_out):
            V.assert_untouched(buf, 1, 0, n, off)                      # never written
        else:
            res[k] = V.check_out(buf, 1, n, n, off)[0]
    return res


def _within(name, got, ref, bar):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    lim = HI * bar + 1e-30
    assert (err <= lim).all(), (name, float((err - lim).max()), int((err > lim).sum()))


CASES = [(B, A, f) for B in BS for A in AS for f in FORMS]


@pytest.mark.parametrize('B,A,form', CASES, ids=[f'B{B}-A{A}-d{f[0]}q{f[1]}' for B, A, f in CASES])
def test_dqn_td(B, A, form):
    dueling, double_q = form
    view = VIEW_NAMES[(BS.index(B) + AS.index(A) + FORMS.index(form)) % len(VIEW_NAMES)]
    c = _case(B, A, dueling, double_q, seed=1000 * B + 10 * A + 2 * dueling + double_q)
    r = _reference(c, A, dueling, double_q, True)
    got = _run(c, A, dueling, double_q, True, view)
    rows = np.arange(B)
    y, td = got['y'].double().numpy(), got['td'].double().numpy()
    # j* through y: the candidate targets of a live row with distinct target scores
    g32 = float(np.float32(GAMMA))
    cand = c['rew'].astype(np.float64)[:, None] + g32 * r['qt']
    sep = np.array([np.diff(np.sort(row)).min() if A > 1 else 1.0 for row in r['qt']])
    live = (c['done'] == 0) & (sep > 0)
    if double_q:
        assert live.sum() >= min(B, 2) - 1 and (sep > 0).all()
    picked = np.abs(cand - y[:, None]).argmin(1)
    assert (picked[live] == r['js'][live]).all()
    term = c['done'] == 1
    assert np.array_equal(got['y'].numpy()[term], c['rew'][term])       # y == r exactly
    _within('y', y, r['y'], r['ey'])
    _within('td', td, r['td'], r['etd'])
    for i, d in zip(c['edge'], (1.0, -1.0, 1.125, 0.875)):
        if c['done'][i] == 1:
            assert td[i] == d, (i, td[i], d)                            # exact rows at the Huber knee
    dadv = got['dadv'].double().numpy()
    _within('dadv', dadv, r['dadv'], r['ed'])
    # g from the kernel's own td_out, in fp32 arithmetic
    t32 = got['td'].numpy()
    g32_ = (c['w'] * np.clip(t32, np.float32(-1), np.float32(1))) / np.float32(B)
    assert g32_.dtype == np.float32
    if dueling:
        assert np.array_equal(got['dval'].numpy().view(np.int32), g32_.view(np.int32))
        _within('dval', got['dval'].double().numpy(), r['g'], r['eg'])
    else:
        mask = np.zeros((B, A), dtype=bool)
        mask[rows, c['act']] = True
        assert (dadv[~mask] == 0).all()                                 # sparsity pattern
        assert np.array_equal(got['dadv'].numpy()[mask].view(np.int32), g32_.view(np.int32))
    st = got['stats'].double().numpy()
    _within('loss', st[0], r['loss'], r['eloss'])
    _within('mean|td|', st[1], r['mtd'], r['emtd'])


@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_dqn_td_null_weights_equal_ones_and_optional_y(form):
    dueling, double_q = form
    B, A = 257, 3
    c = _case(B, A, dueling, double_q, seed=77)
    ones = dict(c, w=np.ones(B, dtype=np.float32))
    a = _run(ones, A, dueling, double_q, True, 'wide3')
    b = _run(ones, A, dueling, double_q, False, 'wide3', y_out=False)
    for k in b:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    r = _reference(c, A, dueling, double_q, False)
    _within('loss', b['stats'].double().numpy()[0], r['loss'], r['eloss'])


def test_dqn_td_clamps_out_of_range_actions():
    """-1, A and 2.5 in the action column are a caller error; the index is
    clamped (0, A - 1, 2), so only the A columns are written: the canaries of
    every output stay intact and the gradient lands in the clamped column"""
    B, A = 6, 4
    c = _case(B, A, 0, 1, seed=5)
    c['act'] = np.array([-1.0, A, 2.5, 1.0, -0.0, 1e9], dtype=np.float32)
    c['rew'] = np.random.RandomState(6).randn(B).astype(np.float32)     # no row with td == 0
    c['done'][:] = 0
    got = _run(c, A, 0, 1, True, 'off1wide3')           # check_out: canaries intact, no NaN
    want = [0, A - 1, 2, 1, 0, A - 1]
    dadv = got['dadv'].numpy()
    for i, j in enumerate(want):
        others = [k for k in range(A) if k != j]
        assert dadv[i, j] != 0 and (dadv[i, others] == 0).all(), (i, dadv[i])
    d = _run(c, A, 1, 1, True, 'off1wide3')
    assert torch.isfinite(d['dadv']).all() and torch.isfinite(d['dval']).all()


SHAPES_G = [(rows, A) for rows in BS for A in AS]


@pytest.mark.parametrize('dueling', [1, 0])
@pytest.mark.parametrize('rows,A', SHAPES_G, ids=[f'{r}x{a}' for r, a in SHAPES_G])
def test_dqn_greedy(rows, A, dueling):
    """the device-side statement of the tie rule: first index of the maximum"""
    view = VIEW_NAMES[(BS.index(rows) + AS.index(A) + dueling) % len(VIEW_NAMES)]
    pad, off = V.VIEWS[view]
    adv, want = _scores(rows, A, np.random.RandomState(rows + A), ties=True)
    if A >= 3:
        assert {int(want[i]) for i in range(min(rows, 7)) if i % 7 in (0, 3, 5)} <= {0, 1}
    val = np.random.RandomState(3).randint(-24, 25, size=rows).astype(np.float32) / 8
    ap, abuf = V.make_in(torch.from_numpy(adv), A + pad, off, DEV)
    vp, vbuf = _col(val, 1 + pad, off)
    out = torch.full((rows + 2,), -7, dtype=torch.int32, device=DEV)
    L.call('smi_dqn_greedy', ap, A + pad, vp if dueling else None, 1 + pad, rows, A, dueling,
           ctypes.c_void_p(out.data_ptr() + 4), _st())
    assert _last() == f'dqn_greedy_kernel<{dueling}>'
    o = out.cpu().numpy()
    assert o[0] == -7 and o[-1] == -7
    assert np.array_equal(o[1:-1], want)


def test_argument_errors():
    lib = L.lib()
    x = torch.zeros(64, device=DEV)
    p = L.ptr(x)
    ok = dict(adv=p, lda=3, adv_n=p, ldn=3, adv_t=p, ldt=3, val=p, vs=1, val_n=p, vns=1, val_t=p,
              vts=1, act=p, as_=1, rew=p, rs=1, done=p, ds=1, w=None, B=4, A=3, gamma=0.99,
              dueling=1, double_q=1, dadv=p, ldd=3, dval=p, td=p, y=None, stats=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.smi_dqn_td(*a.values(), None)
    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(adv=None), dict(adv_t=None), dict(act=None), dict(rew=None), dict(done=None),
           dict(dadv=None), dict(td=None), dict(stats=None), dict(adv_n=None), dict(B=0), dict(A=0),
           dict(lda=2), dict(ldn=2), dict(ldt=2), dict(ldd=2), dict(val=None), dict(val_n=None),
           dict(val_t=None), dict(dval=None)]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
        assert 'dqn_td' in _err(), (kw, _err())
    # the mates are needed only by the forms that read them
    assert call(adv_n=None, val_n=None, ldn=0, double_q=0) == 0
    assert call(val=None, val_n=None, val_t=None, dval=None, dueling=0) == 0
    out = torch.zeros(8, dtype=torch.int32, device=DEV)
    g = lambda *a: lib.smi_dqn_greedy(*a, None)                        # noqa: E731
    assert g(p, 3, p, 1, 4, 3, 1, L.ptr(out)) == 0
    assert g(p, 3, p, 1, 0, 3, 1, L.ptr(out)) == 0
    for a in ((None, 3, p, 1, 4, 3, 1, L.ptr(out)), (p, 3, p, 1, 4, 3, 1, None),
              (p, 3, None, 1, 4, 3, 1, L.ptr(out)), (p, 2, p, 1, 4, 3, 1, L.ptr(out)),
              (p, 3, p, 1, -1, 3, 1, L.ptr(out)), (p, 3, p, 1, 4, 0, 1, L.ptr(out))):
        assert g(*a) == E_ARG and 'dqn_greedy' in _err(), a
    torch.cuda.synchronize()
