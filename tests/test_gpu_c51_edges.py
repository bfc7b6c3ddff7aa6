"""The kernels of dqn_dist_kernels.hip at the edges of their launchers, against fp64.

c51_td_kernel<DUELING, DOUBLE_Q> + c51_stats_kernel and c51_q_kernel<DUELING> through
the C ABI, on the inputs of tests/c51_ref.py (families(); tests/test_cpu_c51_ref.py
shows what they reach), against c51_td_loop in float64 on the project's bar
(_fp32_as_good_as_torch, c51_td in float32 as the fp32 reference).  astar, greedy,
zero patterns and canaries are exact.  Every input lies in a NaN-filled buffer and
every output in a canaried one (tests/views.py); the partials workspace is exactly
smi_dqn_c51_partials_bytes(B) bytes with a canary behind it.  Every launch asserts
smi_last_launch() and, from the pointers it passes, which staging form the host picks.

Which test runs which path:
  staging forms (16-byte with dword tail, padded ld, 4-byte base, one misaligned
  operand of three, A N > 1024 on the 16-byte path, dword second round)
                                    test_td_staging, test_q_staging
  A N == 3072, the LDS ceiling      test_lds_ceiling_td, test_lds_ceiling_q
  rpb > kNW, slot[it & 1], quads past B, c51_stats_kernel with nb > 64
                                    test_row_blocks
  the zero fill of td_all over several grid passes
                                    test_shard_fill
  strides of action / reward / done other than 7
                                    every launch of _td (strides 1, 3, 2 or 5, 1, 4)
  six (with dadv and dval eight) different leading dimensions in one call
                                    test_td_eight_leading_dimensions
  an adv_next the form does not read has no say in the staging form
                                    test_td_staging[...-d0q0-next_off1] (and d1q0)
  m_out / astar_out NULL            test_optional_outputs
  supports, gamma, fractional done, b on an atom, +-inf rewards, ties
                                    test_corners (and the tie rows of every B = 9 family)
  actions outside [0, A)            test_wild_actions
  NaN reward, done, weight, logit   test_nan_*
  SMI_E_ARG branches                test_td_argument_errors, test_shard_argument_errors,
                                    test_q_argument_errors
No row is left out of any comparison: the tie rows' a* is asserted exactly, and with
a* equal everything that depends on it is compared like any other row.
"""

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from tests import c51_ref as C
from tests import views as V
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SMI_E_ARG = -1
FORMS = [(1, 1), (1, 0), (0, 1), (0, 0)]
NAN_BITS = int(torch.tensor([V.NAN]).view(torch.int32))
PART_TAIL = 8                                     # canary doubles behind the partials
SENT64 = 0x7FF5A5A5A5A5A5A5                       # their fill: a NaN no sum of the kernel's has
FAM = C.families()


def last():
    return L.lib().smi_last_launch().decode()


def bits(t):
    t = torch.as_tensor(t).contiguous()
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def _close(name, got, ref32, ref64):
    got, ref32, ref64 = (np.asarray(t.detach() if torch.is_tensor(t) else t, dtype=np.float64)
                         for t in (got, ref32, ref64))
    print(f'{name}: e_gpu {np.abs(got - ref64).max():.3e} e_cpu {np.abs(ref32 - ref64).max():.3e} '
          f'scale {np.abs(ref64).max():.3e}')
    _fp32_as_good_as_torch(got, ref32, ref64)


def _aligned16(ptr, ld):
    return ptr.value % 16 == 0 and ld % 4 == 0


def _layout(view, width):
    """views.layout, or (pad, off) spelled out where a case needs more than the five names"""
    return V.layout(view, width) if isinstance(view, str) else (width + view[0], view[1])


class Out(object):
    """rows x cols floats (or int32) in a canaried buffer"""

    def __init__(self, rows, cols, view='tight', pad=0):
        self.rows, self.cols = rows, cols
        self.ld, self.off = _layout(view, cols + pad)
        self.ptr, self.buf = V.make_out(rows, cols, self.ld, self.off, device=DEV)

    def read(self):
        V.assert_untouched(self.buf, self.rows, self.cols, self.ld, self.off)
        return V.read_out(self.buf, self.rows, self.cols, self.ld, self.off)

    def pristine(self):
        return bool((bits(self.buf.cpu()) == NAN_BITS).all())


def _in(t, width, view):
    """t [rows][width] in a NaN-filled buffer: (pointer, ld, buffer)"""
    ld, off = _layout(view, width)
    ptr, buf = V.make_in(t.reshape(-1, width), ld, off, DEV)
    return ptr, ld, buf


def _col(t, stride, off):
    """t [rows] as column 0 of a NaN-filled [rows][stride] matrix `off` floats into its buffer"""
    ptr, buf = V.make_in(t.reshape(-1, 1), stride, off, DEV)
    return ptr, stride, buf


def _td(kw, form, views=None, weighted=True, c=None, rows=None, shard=None, null=(), over=None,
        strides=(1, 3, 2), expect_error=False, unread=False):
    """rows [lo, hi) of the family (or of its variant c) through smi_dqn_c51_td, or with
    shard = (B_global, row0) through smi_dqn_c51_td_shard.  views: operand -> views.VIEWS name
    (default tight); null: the pointers passed as NULL; over: scalar arguments replaced in the
    call alone; unread: adv_next (and val_next) are handed over, in their views, to a form without
    double-Q too, which must not look at them.  Returns the outputs on the host, 'nb' (the partial slots written) and 'vec'
    (the staging form the pointers ask for); expect_error: the return code, after asserting
    that nothing was launched or written."""
    views, over = views or {}, over or {}
    c = c or C.family(**kw)
    (A, N, v_min, v_max, gamma), (dueling, double_q) = C.params(kw), form
    lo, hi = rows or (0, kw['B'])
    B = hi - lo
    Bg, row0 = shard or (B, 0)
    keep, a = [], {}

    def operand(name, t, width):
        if t is None or name in null:
            a[name], a['ld_' + name] = None, 0          # a leading dimension nobody reads
            return
        a[name], a['ld_' + name], buf = _in(t[lo:hi], width, views.get(name, 'tight'))
        keep.append(buf)
    for name, k in (('adv', 'q'), ('adv_n', 'n'), ('adv_t', 't')):
        operand(name, c[k][0] if (name != 'adv_n' or double_q or unread) else None, A * N)
    for name, k in (('val', 'q'), ('val_n', 'n'), ('val_t', 't')):
        operand(name, c[k][1] if dueling and (name != 'val_n' or double_q or unread) else None, N)
    for i, name in enumerate(('act', 'rew', 'done')):
        if name in null:
            a[name], a['ld_' + name] = None, strides[i]
        else:
            a[name], a['ld_' + name], buf = _col(c[name][lo:hi], strides[i], i)
            keep.append(buf)
    a['w'] = None
    if weighted:
        a['w'], _, buf = _in(c['w'][lo:hi], B, 'off1')
        keep.append(buf)
    o = {'dadv': Out(B, A * N, views.get('dadv', 'tight')), 'dval': Out(B, N, views.get('dval', 'tight')),
         'td': Out(1, Bg, views.get('td', 'tight')), 'm': Out(B, N), 'astar': Out(1, B), 'stats': Out(1, 2)}
    slots = int(L.lib().smi_dqn_c51_partials_bytes(B)) // 16
    assert slots == (B + 3) // 4
    part = torch.full((2 * slots + PART_TAIL,), SENT64, dtype=torch.int64, device=DEV)
    outp = lambda k: None if k in null else o[k].ptr                                    # noqa: E731
    s = dict(B=B, Bg=Bg, row0=row0, A=A, N=N, v_min=v_min, v_max=v_max, gamma=gamma,
             partials_bytes=16 * slots, ldd=o['dadv'].ld, lddv=o['dval'].ld if dueling else 0,
             **{k: v for k, v in a.items() if k.startswith('ld_')})
    s.update(over)
    args = [a['adv'], s['ld_adv'], a['adv_n'], s['ld_adv_n'], a['adv_t'], s['ld_adv_t'],
            a['val'], s['ld_val'], a['val_n'], s['ld_val_n'], a['val_t'], s['ld_val_t'],
            a['act'], s['ld_act'], a['rew'], s['ld_rew'], a['done'], s['ld_done'], a['w'], s['B']]
    args += [s['Bg'], s['row0']] if shard else []
    args += [s['A'], s['N'], s['v_min'], s['v_max'], s['gamma'], dueling, double_q, outp('dadv'), s['ldd'],
             outp('dval') if dueling else None, s['lddv'], outp('td'), outp('m'),
             outp('astar'), None if 'partials' in null else L.ptr(part), s['partials_bytes'],
             outp('stats'), L.stream()]
    name = 'smi_dqn_c51_td_shard' if shard else 'smi_dqn_c51_td'
    before = last()
    rc = getattr(L.lib(), name)(*args)
    torch.cuda.synchronize()
    if expect_error:
        assert last() == before, 'a rejected call launched'
        assert all(x.pristine() for x in o.values()) and bool((part == SENT64).all())
        return rc
    L.check(rc, name)
    assert last() == f'c51_td_kernel<{dueling},{double_q}>'
    res = {k: x.read() for k, x in o.items() if k not in null and (k != 'dval' or dueling)}
    for k in null:
        if k in o:
            assert o[k].pristine(), k
    if not dueling:
        assert o['dval'].pristine()
    res['td'] = res['td'].reshape(-1)
    res['stats'] = res['stats'].reshape(-1)
    if 'astar' in res:
        res['astar'] = bits(res['astar']).reshape(-1)
    written = part.cpu() != SENT64
    res['nb'] = int(written[:2 * slots].sum()) // 2
    assert bool(written[:2 * res['nb']].all()) and not bool(written[2 * res['nb']:].any())
    read = ['adv', 'adv_t'] + (['adv_n'] if double_q else [])
    res['vec'] = all(_aligned16(a[k], a['ld_' + k]) for k in read)
    return res


def _check(got, kw, form, weighted, c=None, B_global=None, row0=0):
    """every output against the loop reference in float64 on the project's bar; a* exactly"""
    r32, _, r64 = (C.refs(kw, form[1], weighted, B_global) if c is None
                   else C.refs_of(c, kw, form[1], weighted, B_global))
    assert np.array_equal(got['astar'].numpy(), r64['astar'])
    td = got['td'][row0:row0 + kw['B']]
    for k, v in (('m', got['m']), ('td', td), ('dadv', got['dadv']), ('stats', got['stats'])) + \
            ((('dval', got['dval']),) if form[0] else ()):
        _close(k, v, r32[k], r64[k])


# ------------------------------------------------------------ staging matrix
def _view_case(name):
    """operand -> view: `name` on the three score slabs; val*, dadv and dval each take another"""
    names = sorted(V.VIEWS)
    if name in V.VIEWS:
        rot = lambda k: names[(names.index(name) + k) % len(names)]                     # noqa: E731
        v = {k: name for k in ('adv', 'adv_n', 'adv_t')}
        v.update({k: rot(1) for k in ('val', 'val_n', 'val_t')}, dadv=rot(2), dval=rot(3), td=rot(4))
        return v
    return {{'next_off1': 'adv_n', 'target_off1': 'adv_t'}[name]: 'off1', 'dadv': 'wide3', 'val': 'off1wide3'}


def _wants_vec(A, N, name, double_q):
    """the 16-byte form: every score slab the form reads at offset 0 with ld % 4 == 0"""
    if name in V.VIEWS:
        pad, off = V.VIEWS[name]
        return off == 0 and (A * N + pad) % 4 == 0
    return (A * N) % 4 == 0 and name == 'next_off1' and not double_q


STAGE_VIEWS = sorted(V.VIEWS) + ['next_off1', 'target_off1']
STAGE_TD = [(A, N, f, v) for A, N in C.STAGE_SHAPES for f in (FORMS if (A, N) == (3, 51) else [(1, 1), (0, 0)])
            for v in STAGE_VIEWS]


def test_staging_matrix_reaches_every_form():
    """153 and 165 with a dword tail behind 16-byte loads, 1088 in two 16-byte rounds, 306 in two
    dword rounds, one misaligned operand of three, and the operand a form does not read"""
    vec = {(A * N, v, f[1]): _wants_vec(A, N, v, f[1]) for A, N, f, v in STAGE_TD}
    assert vec[153, 'wide3', 1] and vec[165, 'wide3', 0] and vec[1088, 'tight', 1] and vec[4, 'wide4', 0]
    assert not any(v for (an, _, _), v in vec.items() if an == 306)
    assert not vec[1088, 'off1', 1] and not vec[1088, 'target_off1', 0] and not vec[1088, 'next_off1', 1]
    assert vec[1088, 'next_off1', 0]


@pytest.mark.parametrize('A,N,form,view', STAGE_TD,
                         ids=[f'{A}x{N}-d{f[0]}q{f[1]}-{v}' for A, N, f, v in STAGE_TD])
def test_td_staging(A, N, form, view):
    kw = FAM[f'stage-{A}x{N}-d{form[0]}']
    weighted = (A + len(view) + form[1]) % 2 == 0
    # next_off1 without double-Q: the misaligned adv_next is passed and must have no say
    got = _td(kw, form, _view_case(view), weighted, strides=(5, 1, 4) if weighted else (1, 3, 2),
              unread=view == 'next_off1')
    assert got['vec'] == _wants_vec(A, N, view, form[1]) and got['nb'] == 3
    _check(got, kw, form, weighted)


def test_td_eight_leading_dimensions():
    """lda, ldn, ldt, ldv, ldvn, ldvt, ldd and lddv pairwise distinct in one dueling + double-Q
    call: an operand read with a neighbour's leading dimension lands in NaN padding or in
    another row"""
    kw, form = FAM['stage-5x33-d1'], (1, 1)
    views = {'adv': 'tight', 'adv_n': 'wide3', 'adv_t': 'wide4', 'val': 'wide4', 'val_n': 'tight',
             'val_t': 'wide3', 'dadv': (7, 1), 'dval': (5, 0)}
    lds = [_layout(views[k], 33 if 'val' in k else 165)[0] for k in sorted(views)]
    assert sorted(lds) == [33, 36, 37, 38, 165, 168, 169, 172]
    for weighted in (True, False):
        got = _td(kw, form, views, weighted)
        assert not got['vec']                       # lda = 165
        _check(got, kw, form, weighted)
    views.update(adv='wide3', adv_n=(11, 0), adv_t=(7, 0))     # 168, 176, 172: 16-byte form
    views.update(dadv=(8, 1))
    lds = [_layout(views[k], 33 if 'val' in k else 165)[0] for k in sorted(views)]
    assert len(set(lds)) == 8
    got = _td(kw, form, views, True)
    assert got['vec']
    _check(got, kw, form, True)


def _q(kw, dueling, view='tight', rows=None, null=(), over=None, expect_error=False):
    """smi_dqn_c51_q on the family's target net (its Q(s') holds the tie rows), ldq = A + 2"""
    c, (A, N, v_min, v_max, _), over = C.family(**kw), C.params(kw), over or {}
    rows = kw['B'] if rows is None else rows
    names = sorted(V.VIEWS)
    adv, lda, b0 = _in(c['t'][0], A * N, view)
    val, ldv, b1 = _in(c['t'][1], N, names[(names.index(view) + 1) % len(names)]) if dueling else (None, 0, None)
    q, greedy = Out(kw['B'], A, names[(names.index(view) + 2) % len(names)], pad=2), Out(1, kw['B'])
    s = dict(lda=lda, ldv=ldv, rows=rows, A=A, N=N, v_min=v_min, v_max=v_max, ldq=q.ld)
    s.update(over)
    before = last()
    rc = L.lib().smi_dqn_c51_q(None if 'adv' in null else adv, s['lda'], None if 'val' in null else val,
                               s['ldv'], s['rows'], s['A'], s['N'], s['v_min'], s['v_max'], dueling,
                               None if 'q' in null else q.ptr, s['ldq'],
                               None if 'greedy' in null else greedy.ptr, L.stream())
    torch.cuda.synchronize()
    if expect_error or rows == 0:
        assert last() == before and q.pristine() and greedy.pristine()
        return rc
    L.check(rc, 'smi_dqn_c51_q')
    assert last() == f'c51_q_kernel<{dueling}>'
    res = {'q': q.read(), 'vec': _aligned16(adv, lda)}
    if 'greedy' in null:
        assert greedy.pristine()
    else:
        res['greedy'] = bits(greedy.read()).reshape(-1)
    return res


def _check_q(got, kw):
    r32, _, r64 = C.refs(kw, 0, 0)                   # without double-Q q_sel is the target net's
    _close('q', got['q'], r32['q_sel'], r64['q_sel'])
    assert np.array_equal(got['greedy'].numpy(), r64['astar'])


@pytest.mark.parametrize('view', sorted(V.VIEWS))
@pytest.mark.parametrize('dueling', [1, 0])
@pytest.mark.parametrize('A,N', C.STAGE_SHAPES)
def test_q_staging(A, N, dueling, view):
    kw = FAM[f'stage-{A}x{N}-d{dueling}']
    got = _q(kw, dueling, view)
    assert got['vec'] == _wants_vec(A, N, view, 0)
    _check_q(got, kw)


# --------------------------------------------------------------- LDS ceiling
@pytest.mark.parametrize('form', [(1, 1), (0, 0)], ids=['d1q1', 'd0q0'])
def test_lds_ceiling_td(form):
    kw = FAM[f'lds-48x64-d{form[0]}']
    assert kw['A'] * kw['N'] == 3072
    got = _td(kw, form, weighted=bool(form[0]))
    assert got['vec'] and got['nb'] == 2
    _check(got, kw, form, bool(form[0]))


@pytest.mark.parametrize('dueling', [1, 0])
def test_lds_ceiling_q(dueling):
    kw = FAM[f'lds-48x64-d{dueling}']
    _check_q(_q(kw, dueling), kw)


# ---------------------------------------------------------------- row blocks
@pytest.mark.parametrize('weighted', [True, False], ids=['w', 'now'])
@pytest.mark.parametrize('which', [0, 1], ids=['two-quads', 'three-quads'])
def test_row_blocks(which, weighted):
    """B = 16 CUs + 1: two quads of rows per workgroup, the last workgroup holds one row;
    B = 32 CUs + 5: three quads, the last workgroup's second and third lie past B.  Both
    give c51_stats_kernel more than 64 slots."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, rpb = C.row_block_sizes(cus)[which], (8, 12)[which]
    kw, form = dict(B=B, A=2, N=3, dueling=1, seed=1), (1, 1)
    got = _td(kw, form, {'dadv': 'wide3', 'adv': 'wide4'}, weighted)
    assert got['nb'] == (B + rpb - 1) // rpb and got['nb'] > 64 and B - (got['nb'] - 1) * rpb == 1
    _check(got, kw, form, weighted)
    # the statistics: the fp64 sum of the kernel's own fp32 td and w * td, rounded once
    td = got['td']
    wtd = (C.family(**kw)['w'] * td) if weighted else td
    for i, terms in enumerate((wtd, td)):
        want = np.float32(terms.double().sum().item() / B)
        assert abs(float(got['stats'][i]) - float(want)) <= float(np.spacing(want)), i
    # the first 64 rows alone: one quad per workgroup, the same bits
    head = _td(kw, form, {'dadv': 'wide3', 'adv': 'wide4'}, weighted, rows=(0, 64))
    assert head['nb'] == 16
    assert same_bits(head['m'], got['m'][:64]) and same_bits(head['td'], td[:64])
    assert torch.equal(head['astar'], got['astar'][:64])
    if B & (B - 1) == 0:                             # g / 64 and g / B differ by a power of two
        for k in ('dadv', 'dval'):
            assert same_bits(head[k], got[k][:64] * (B / 64.0)), k


# ---------------------------------------------------------------- shard fill
@pytest.mark.parametrize('row0', [0, 300, 4 + 3 * 256 + 7 - 4])
def test_shard_fill(row0):
    """one workgroup of 256 threads clears B_global - B = 775 entries: four passes"""
    kw, form, Bg = FAM['shard'], (1, 1), 4 + 3 * 256 + 7
    got = _td(kw, form, {'td': 'off1', 'dadv': 'wide3'}, True, shard=(Bg, row0))
    assert got['nb'] == 1
    outside = torch.cat([got['td'][:row0], got['td'][row0 + 4:]])
    assert outside.numel() == Bg - 4 and bool((bits(outside) == 0).all())           # +0.0f
    whole = _td(kw, form, {'dadv': 'wide3'}, True)
    assert same_bits(got['td'][row0:row0 + 4], whole['td']) and same_bits(got['m'], whole['m'])
    assert torch.equal(got['astar'], whole['astar'])
    _check(got, kw, form, True, B_global=Bg, row0=row0)


# ------------------------------------------------- the specification's corners
CORNERS = sorted(n for n in FAM if n.startswith('corner'))


@pytest.mark.parametrize('double_q', [1, 0])
@pytest.mark.parametrize('name', CORNERS)
def test_corners(name, double_q):
    """supports that are asymmetric or have a non-dyadic D, gamma 0 / 1 / fp32(0.99), d = 0.5,
    r = k D and (k + 1/2) D, r = +-inf, two- and three-way ties of Q(s')"""
    kw = FAM[name]
    form, weighted = (kw['dueling'], double_q), bool(double_q)
    got = _td(kw, form, {'adv_t': 'wide3', 'dval': 'off1'}, weighted)
    _check(got, kw, form, weighted)
    ties = C.tie_rows(kw['B'], kw['A'])
    assert [int(got['astar'][r]) for r in sorted(ties)] == [ties[r][0] for r in sorted(ties)]


@pytest.mark.parametrize('form', [(1, 1), (0, 0)], ids=['d1q1', 'd0q0'])
def test_wild_actions(form):
    """-1, A, A + 0.5, 1.9, NaN, 1e9: the reference at dqn_action_index's clamp, nothing outside
    the A actions' columns written (the canaries of a padded dadv)"""
    kw = FAM[f'stage-3x51-d{form[0]}']
    c = dict(C.family(**kw))
    c['act'] = torch.tensor([-1.0, 3.0, 3.5, 1.9, V.NAN, 1e9, 0.0, 2.0, 1.0])
    got = _td(kw, form, {'dadv': 'off1wide3', 'dval': 'wide4'}, True, c=c)
    _check(got, kw, form, True, c=c)
    clamped = dict(c, act=C.action_index(c['act'], 3).float())
    again = _td(kw, form, {'dadv': 'off1wide3', 'dval': 'wide4'}, True, c=clamped)
    assert all(same_bits(got[k], again[k]) for k in ('dadv', 'td', 'm', 'stats'))


# ----------------------------------------------------------------------- NaN
NAN_ROW = 3
NAN_FORMS = pytest.mark.parametrize('form', [(1, 1), (0, 0)], ids=['d1q1', 'd0q0'])


def _nan_pair(form, change):
    """(clean run, run of the inputs `change` has put a NaN into, loop reference of those)"""
    kw = FAM[f'stage-3x51-d{form[0]}']
    c = {k: (tuple(None if t is None else t.clone() for t in v) if isinstance(v, tuple) else
             v.clone() if torch.is_tensor(v) else v) for k, v in C.family(**kw).items()}
    change(c)
    views = {'dadv': 'wide3', 'adv': 'wide4'}
    bad = _td(kw, form, views, True, c=c)
    return _td(kw, form, views, True), bad, C.refs_of(c, kw, form[1], True)[2], c


def _others_keep_their_bits(clean, bad, keys):
    rest = [n for n in range(9) if n != NAN_ROW]
    for k in keys:
        assert same_bits(clean[k][rest], bad[k][rest]), k
    assert torch.equal(clean['astar'], bad['astar'])


@NAN_FORMS
@pytest.mark.parametrize('which', ['rew', 'done'])
def test_nan_reward_or_done(which, form):
    """Tz's clamp hands the NaN on: the row's m, td and gradients are NaN as in the reference
    (never a finite loss for the sum tree), both statistics too, no other row moves"""
    def change(c):
        c[which][NAN_ROW] = V.NAN
    clean, bad, ref, _ = _nan_pair(form, change)
    keys = ('m', 'td', 'dadv') + (('dval',) if form[0] else ())
    for k in keys:
        print(f'NaN {which}: {k}[{NAN_ROW}] kernel {bad[k][NAN_ROW].numpy().reshape(-1)[:3]} '
              f'reference {np.asarray(ref[k][NAN_ROW]).reshape(-1)[:3]}')
    for k in keys:
        assert np.array_equal(np.isnan(bad[k][NAN_ROW].numpy()), np.isnan(ref[k][NAN_ROW])), k
    assert np.isnan(ref['m'][NAN_ROW]).all() and np.isnan(ref['td'][NAN_ROW])
    assert bool(torch.isnan(bad['stats']).all())
    _others_keep_their_bits(clean, bad, keys)


@NAN_FORMS
def test_nan_weight(form):
    def change(c):
        c['w'][NAN_ROW] = V.NAN
    clean, bad, ref, _ = _nan_pair(form, change)
    assert np.array_equal(np.isnan(bad['dadv'][NAN_ROW].numpy()), np.isnan(ref['dadv'][NAN_ROW]))
    assert np.isnan(ref['dadv'][NAN_ROW]).any()
    assert same_bits(bad['td'], clean['td']) and same_bits(bad['m'], clean['m'])
    assert bool(torch.isnan(bad['stats'][0])) and same_bits(bad['stats'][1], clean['stats'][1])
    _others_keep_their_bits(clean, bad, ('dadv',) + (('dval',) if form[0] else ()))


@NAN_FORMS
def test_nan_online_logit_of_the_action_taken(form):
    def change(c):
        ai = int(c['act'][NAN_ROW])
        c['q'][0][NAN_ROW, ai * 51 + 7] = V.NAN
    clean, bad, ref, c = _nan_pair(form, change)
    ai = int(c['act'][NAN_ROW])
    assert bool(torch.isnan(bad['td'][NAN_ROW])) and np.isnan(ref['td'][NAN_ROW])
    assert bool(torch.isnan(bad['dadv'][NAN_ROW, ai * 51:(ai + 1) * 51]).all())
    assert same_bits(bad['m'], clean['m'])
    _others_keep_their_bits(clean, bad, ('td', 'dadv') + (('dval',) if form[0] else ()))


# ------------------------------------------------------------ optional outputs
@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_optional_outputs(form):
    kw = FAM[f'stage-5x33-d{form[0]}']
    full = _td(kw, form, {'adv': 'wide3'}, True)
    for null in (('m', 'astar'), ('m',), ('astar',)):
        part = _td(kw, form, {'adv': 'wide3'}, True, null=null)
        for k in ('dadv', 'dval', 'td', 'm', 'astar', 'stats'):
            if k in part:
                assert same_bits(part[k], full[k]), (null, k)
        assert not any(k in part for k in null)


# ------------------------------------------------------------ argument errors
def _rejected(rc, word):
    msg = L.lib().smi_last_error().decode()
    assert rc == SMI_E_ARG and word in msg, (rc, msg)


def _launch_something_else(kw, dueling=1):
    _q(kw, dueling)                                 # smi_last_launch now names the q kernel


@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_td_argument_errors(form):
    dueling, double_q = form
    kw = FAM[f'stage-3x51-d{dueling}']
    _launch_something_else(kw, dueling)
    bad = lambda word, **k: _rejected(_td(kw, form, expect_error=True, **k), word)      # noqa: E731
    bad('atoms', over={'N': 1})
    bad('atoms', over={'N': 65})
    bad('A < 1', over={'A': 0})
    bad('3072', over={'A': 49, 'N': 64})
    bad('3072', over={'A': 100, 'N': 51})
    bad('3072', over={'A': 439, 'N': 7})            # 3073: one past the ceiling
    bad('v_max', over={'v_max': -10.0})
    bad('v_max', over={'v_max': -11.0})
    bad('v_max', over={'v_max': V.NAN})
    bad('B < 1', over={'B': 0})
    bad('partials', over={'partials_bytes': 32})    # three slots of 16 bytes needed
    reads = {'ld_adv': 1, 'ld_adv_t': 1, 'ldd': 1, 'ld_adv_n': double_q, 'ld_val': dueling,
             'ld_val_t': dueling, 'lddv': dueling, 'ld_val_n': dueling and double_q}
    for name, read in reads.items():
        width = 51 if 'val' in name or name == 'lddv' else 153
        if read:
            bad('leading', over={name: width - 1})
    need = {'adv': 1, 'adv_t': 1, 'act': 1, 'rew': 1, 'done': 1, 'dadv': 1, 'td': 1, 'partials': 1,
            'stats': 1, 'adv_n': double_q, 'val': dueling, 'val_t': dueling, 'dval': dueling,
            'val_n': dueling and double_q}
    for name, needed in need.items():
        if needed:
            bad('null' if name in ('adv', 'adv_t', 'act', 'rew', 'done', 'dadv', 'td', 'partials', 'stats',
                                   'adv_n') else 'dueling needs', null=(name,))


@pytest.mark.parametrize('form', [(1, 0), (0, 1), (0, 0)], ids=['d1q0', 'd0q1', 'd0q0'])
def test_td_accepts_what_the_form_does_not_read(form):
    """the operands of the other forms are NULL with leading dimension 0 in every call of _td;
    here their leading dimensions are one below the minimum of the forms that read them"""
    dueling, double_q = form
    kw = FAM[f'stage-3x51-d{dueling}']
    plain = _td(kw, form)
    over = {'lddv': 50} if not dueling else {}
    over.update({} if double_q else {'ld_adv_n': 152, 'ld_val_n': 50})
    other = _td(kw, form, over=over)
    assert all(same_bits(plain[k], other[k]) for k in ('dadv', 'td', 'm', 'astar', 'stats'))


def test_shard_argument_errors():
    kw, form = FAM['shard'], (1, 1)
    _launch_something_else(FAM['stage-2x2-d1'])
    bad = lambda word, **k: _rejected(_td(kw, form, expect_error=True, **k), word)      # noqa: E731
    bad('row0 < 0', shard=(16, 0), over={'row0': -1})
    bad('row0 + B', shard=(16, 0), over={'row0': 13})
    bad('B_global < B', shard=(16, 0), over={'Bg': 3})
    bad('B < 1', shard=(16, 0), over={'B': 0})
    bad('atoms', shard=(16, 0), over={'N': 65})
    bad('null', shard=(16, 0), null=('td',))
    bad('null', shard=(16, 0), null=('adv_n',))
    bad('dueling needs', shard=(16, 0), null=('val_n',))
    bad('partials', shard=(16, 0), over={'partials_bytes': 15})
    bad('leading', shard=(16, 0), over={'ld_adv_t': 152})


@pytest.mark.parametrize('dueling', [1, 0])
def test_q_argument_errors(dueling):
    kw = FAM[f'stage-3x51-d{dueling}']
    _td(kw, (dueling, 0))                            # smi_last_launch now names the TD kernel
    bad = lambda word, **k: _rejected(_q(kw, dueling, expect_error=True, **k), word)    # noqa: E731
    bad('atoms', over={'N': 1})
    bad('atoms', over={'N': 65})
    bad('A < 1', over={'A': 0})
    bad('3072', over={'A': 49, 'N': 64})
    bad('3072', over={'A': 439, 'N': 7})
    bad('v_max', over={'v_max': -10.0})
    bad('v_max', over={'v_max': V.NAN})
    bad('rows < 0', over={'rows': -1})
    bad('leading', over={'lda': 152})
    bad('leading', over={'ldq': 2})
    bad('null', null=('adv',))
    bad('null', null=('q',))
    if dueling:
        bad('leading', over={'ldv': 50})
        bad('dueling needs', null=('val',))
    else:
        _check_q(_q(kw, 0, over={'ldv': 0}), kw)     # a val stride nobody reads
    assert _q(kw, dueling, rows=0) == 0              # SMI_OK, nothing launched, nothing written
    assert 'greedy' not in _q(kw, dueling, null=('greedy',))
