"""Categorical (C51) DQN references on the CPU, and the inputs of the GPU tests.

  c51_td        plain torch, dtype-generic: the textbook floor / ceil index_add_
                projection and log_softmax, deliberately not the gather form of
                dqn_dist_kernels.hip
  c51_td_loop   float64, one Python loop per row and per atom: the gather form
                max(0, 1 - |b_j - i|), logsumexp written out, the gradients from the
                closed form of the kernel's header; no torch op, no scatter
  family        the seeded inputs tests/test_gpu_c51_edges.py runs, families() their list;
                tests/test_cpu_c51_ref.py checks the two references against each other
                and the conditions on the inputs

Both references: a NaN reward or done makes the row's m (and what follows from it) NaN and
leaves the other rows alone; the action column goes through dqn_action_index's clamp."""
import functools
import math

import numpy as np
import torch
import torch.nn as nn

from tests.dqn_ref import FFQfuncRef

GAMMA = float(np.float32(0.99))


def twin(D, A, N, hidden, dueling):
    """FFQfuncRef with categorical heads: streams(x) = (adv [B][A N], val [B][N] | None)"""
    net = FFQfuncRef(D, A * N, hidden, dueling)
    if dueling:
        net.fc_state_layers[-1] = nn.Linear(hidden[-1], N)
    return net


def logits(adv, val, A, N):
    l = adv.reshape(-1, A, N)
    return l if val is None else (l - l.mean(dim=1, keepdim=True)) + val[:, None, :]


def support(N, v_min, v_max, dtype):
    delta = torch.tensor(v_max - v_min, dtype=dtype) / (N - 1)
    return v_min + torch.arange(N, dtype=dtype) * delta, delta


def expected_q(adv, val, A, N, v_min, v_max):
    return (torch.softmax(logits(adv, val, A, N), 2) * support(N, v_min, v_max, adv.dtype)[0]).sum(2)


def action_index(actions, A):
    """dqn_action_index (dqn_rows.hpp) on a float tensor: negative or NaN -> 0, >= A -> A - 1,
    fractions truncated"""
    a = torch.nan_to_num(actions.reshape(-1).double(), nan=0.0)
    return a.clamp(0, A - 1).floor().long()


def c51_td(online, nxt, target, actions, rewards, dones, w, A, N, v_min, v_max, gamma):
    """online / nxt (None without double-Q) / target: (adv, val | None) at s, s', s'.
    q_sel is the selecting net's Q(s'), td the row losses, objective mean(w td)."""
    dt = online[0].dtype
    B, rows = online[0].shape[0], torch.arange(online[0].shape[0])
    z, delta = support(N, v_min, v_max, dt)
    with torch.no_grad():
        q_sel = expected_q(*(nxt or target), A, N, v_min, v_max)
        astar = q_sel.argmax(1)                                 # the first maximum
        pt = torch.softmax(logits(*target, A, N), 2)[rows, astar]
        r, d = rewards.reshape(B, 1).to(dt), dones.reshape(B, 1).to(dt)
        tz = (r + gamma * ((1 - d) * z)).clamp(v_min, v_max)    # torch.clamp hands a NaN on
        nan = torch.isnan(tz).any(1)                            # a NaN r or d: the whole row
        b = torch.where(nan[:, None], torch.zeros((), dtype=dt), ((tz - v_min) / delta).clamp(0, N - 1))
        lo, up = b.floor(), b.ceil()
        off = (rows * N)[:, None]
        m = torch.zeros(B * N, dtype=dt)
        m.index_add_(0, (lo.long() + off).reshape(-1), (pt * ((up - b) + (lo == up).to(dt))).reshape(-1))
        m.index_add_(0, (up.long() + off).reshape(-1), (pt * (b - lo)).reshape(-1))
        m = m.view(B, N)
        m[nan] = float('nan')
    logp = torch.log_softmax(logits(*online, A, N), 2)[rows, action_index(actions, A)]
    td = -(m * logp).sum(1)
    wv = torch.ones(B, dtype=dt) if w is None else w.reshape(B).to(dt)
    return {'q_sel': q_sel, 'astar': astar, 'm': m, 'td': td.detach(), 'objective': (wv * td).sum() / B,
            'stats': torch.stack([(wv * td).sum() / B, td.sum() / B]).detach()}


# ------------------------------------------------------------ the loop form
def _f64(t):
    if t is None:
        return None
    return np.asarray(t.detach() if torch.is_tensor(t) else t, dtype=np.float64)


def _clamp(x, lo, hi):
    return x if x != x else min(max(x, lo), hi)


def _row_logits(adv, val, A, N):
    """l[a][i] of one row (lists of Python floats, i.e. IEEE doubles)"""
    if val is None:
        return [[adv[a * N + i] for i in range(N)] for a in range(A)]
    mean = []
    for i in range(N):
        s = 0.0
        for a in range(A):
            s += adv[a * N + i]
        mean.append(s / A)
    return [[(adv[a * N + i] - mean[i]) + val[i] for i in range(N)] for a in range(A)]


def _log_softmax(l):
    mx = l[0]
    for x in l[1:]:
        if x > mx:
            mx = x
    s = 0.0
    for x in l:
        s += math.exp(x - mx)
    lse = mx + math.log(s)
    return [x - lse for x in l]


def _expected(l, z):
    q = 0.0
    for lp, zi in zip(_log_softmax(l), z):
        q += zi * math.exp(lp)
    return q


def _first_argmax(q):
    best = 0
    for a in range(1, len(q)):
        if q[a] > q[best]:
            best = a
    return best


def _support_list(N, v_min, v_max):
    D = (v_max - v_min) / (N - 1)
    return [v_min + i * D for i in range(N)], D


def expected_q_loop(adv, val, A, N, v_min, v_max):
    """(q [rows][A] float64, first arg-max [rows]) by plain loops"""
    adv, val = _f64(adv), _f64(val)
    z, _ = _support_list(N, v_min, v_max)
    q = [[_expected(l, z) for l in _row_logits(adv[n].tolist(), None if val is None else val[n].tolist(), A, N)]
         for n in range(adv.shape[0])]
    return np.array(q).reshape(adv.shape[0], A), np.array([_first_argmax(r) for r in q], dtype=np.int64)


def c51_td_loop(online, nxt, target, actions, rewards, dones, w, A, N, v_min, v_max, gamma, B_global=None):
    """c51_td's arguments (tensors or arrays of any float type, widened to float64); B_global
    divides the gradients and the statistics of a shard.  Returns float64 arrays: q_sel, astar,
    tz (before the clamp), b, m, td, dadv, dval (None without dueling), stats."""
    online, target = tuple(map(_f64, online)), tuple(map(_f64, target))
    nxt = None if nxt is None else tuple(map(_f64, nxt))
    act, rew, done = (_f64(t).reshape(-1).tolist() for t in (actions, rewards, dones))
    B = online[0].shape[0]
    Bg = float(B if B_global is None else B_global)
    wl = [1.0] * B if w is None else _f64(w).reshape(-1).tolist()
    z, D = _support_list(N, v_min, v_max)
    row = lambda pr, n: (pr[0][n].tolist(), None if pr[1] is None else pr[1][n].tolist())   # noqa: E731
    out = {k: [] for k in ('q_sel', 'astar', 'tz', 'b', 'm', 'td', 'dadv', 'dval')}
    sum_wl = sum_l = 0.0
    for n in range(B):
        lt = _row_logits(*row(target, n), A, N)
        q_sel = [_expected(l, z) for l in (lt if nxt is None else _row_logits(*row(nxt, n), A, N))]
        astar = _first_argmax(q_sel)
        pt = [math.exp(x) for x in _log_softmax(lt[astar])]
        tz = [rew[n] + gamma * ((1.0 - done[n]) * zj) for zj in z]
        b = [_clamp((_clamp(t, v_min, v_max) - v_min) / D, 0.0, N - 1.0) for t in tz]
        m = []
        for i in range(N):
            s = 0.0
            for j in range(N):
                hat = 1.0 - abs(b[j] - i)
                s += pt[j] * (hat if hat != hat or hat > 0.0 else 0.0)
            m.append(s)
        af = act[n]
        ai = 0 if not af >= 0.0 else (int(af) if af < A else A - 1)
        logp = _log_softmax(_row_logits(*row(online, n), A, N)[ai])
        loss = 0.0
        for i in range(N):
            loss -= m[i] * logp[i]
        g = [wl[n] * (math.exp(logp[i]) - m[i]) / Bg for i in range(N)]
        if online[1] is None:
            dadv = [g[i] if a == ai else 0.0 for a in range(A) for i in range(N)]
        else:
            dadv = [g[i] * ((1.0 if a == ai else 0.0) - 1.0 / A) for a in range(A) for i in range(N)]
        sum_wl += wl[n] * loss
        sum_l += loss
        for k, v in (('q_sel', q_sel), ('astar', astar), ('tz', tz), ('b', b), ('m', m), ('td', loss),
                     ('dadv', dadv), ('dval', g)):
            out[k].append(v)
    res = {k: np.array(v, dtype=np.int64 if k == 'astar' else np.float64) for k, v in out.items()}
    if online[1] is None:
        res['dval'] = None
    res['stats'] = np.array([sum_wl / Bg, sum_l / Bg])
    return res


# ------------------------------------------------- inputs of the GPU tests
def edge_rewards(N, v_min, v_max):
    """(r_int, r_half): float32 rewards v_min + k D and v_min + (k + 1/2) D whose
    b = (r - v_min) / D is exactly k and k + 1/2 in float64 (an interior k where one exists)"""
    D = (v_max - v_min) / (N - 1)
    found = []
    for frac, ks in ((0.0, list(range(1, N - 1)) + [0]), (0.5, range(N - 1))):
        r = next(float(np.float32(v_min + (k + frac) * D)) for k in ks
                 if (float(np.float32(v_min + (k + frac) * D)) - v_min) / D == k + frac)
        found.append(r)
    return tuple(found)


def tie_rows(B, A):
    """{row: the actions with bit-identical logits in the nets at s'} (at most 3 rows)"""
    if B < 8 or A < 2:
        return {}
    return {5: (0, A - 1), 6: (0, 1, A - 1) if A >= 3 else (0, A - 1), 7: (A - 2, A - 1)}


def family(**kw):
    """the inputs of _family(**kw), every tensor a fresh copy: a test may write into them"""
    copy = lambda v: (tuple(None if t is None else t.clone() for t in v) if isinstance(v, tuple)   # noqa: E731
                      else v.clone() if torch.is_tensor(v) else dict(v))
    return {k: copy(v) for k, v in _family(**kw).items()}


@functools.lru_cache(maxsize=None)
def _family(B, A, N, dueling, v_min=-10.0, v_max=10.0, gamma=GAMMA, seed=0, done_half=False, inf=False):
    """N(0, 1) logits with +100 on every second row; action, reward, done, weight columns.
    Row 0 / 1: r = r_int / r_half of edge_rewards with Tz_j = r for every j (terminal, or
    gamma = 0); row 2 / 3: Tz straddles v_max / v_min (lies 0.3 D beyond it with gamma = 0);
    row 4: terminal; tie_rows(B, A): the tied actions carry the largest Q(s') of both nets;
    done_half: d = 0.5 on rows 5, 7, ...; inf: r = -inf, +inf on the last two rows.
    Cached: family() hands out copies."""
    g = torch.Generator().manual_seed(seed)
    c = {'ties': tie_rows(B, A)}
    for k in 'qnt':
        adv, val = torch.randn(B, A * N, generator=g), torch.randn(B, N, generator=g)
        (val if dueling else adv)[1::2] += 100.0
        if k in 'nt':
            for row, acts in c['ties'].items():
                base = adv[row, acts[0] * N:(acts[0] + 1) * N].clone()
                base[N - 1] += 30.0                             # the mass on the top atom
                for a in acts:
                    adv[row, a * N:(a + 1) * N] = base
        c[k] = (adv, val if dueling else None)
    span, mid, D = v_max - v_min, 0.5 * (v_min + v_max), (v_max - v_min) / (N - 1)
    rew = mid + span / 8 * torch.randn(B, generator=g)
    done = (torch.rand(B, generator=g) < 0.2).float()
    act = torch.randint(0, A, (B,), generator=g).float()
    r_int, r_half = edge_rewards(N, v_min, v_max)
    rew[0], rew[1] = r_int, r_half
    done[0:2] = 0.0 if gamma == 0.0 else 1.0
    rew[2], rew[3] = v_max - gamma * mid + 0.3 * D, v_min - gamma * mid - 0.3 * D
    done[2:4] = 0.0
    if B > 4:
        done[4] = 1.0
    if done_half:
        done[5::2] = 0.5
    if inf:
        rew[B - 2], rew[B - 1] = -math.inf, math.inf
    c.update(act=act, rew=rew, done=done, w=0.3 + 0.7 * torch.rand(B, generator=g))
    return c


def gap_ok(q64, skip=()):
    """the condition on the inputs: outside the designated tie rows no fp64 arg-max within 1e-4
    of a tie"""
    q64 = torch.as_tensor(q64)
    keep = torch.ones(q64.shape[0], dtype=torch.bool)
    keep[list(skip)] = False
    return q64.shape[1] == 1 or float(q64[keep].topk(2, 1).values.diff(dim=1).abs().min()) >= 1e-4


def row_block_sizes(cus):
    """B at which a workgroup of c51_td_kernel owns two quads of rows with the last workgroup
    holding one row, and three quads with the last workgroup's other quads wholly past B"""
    return 16 * cus + 1, 32 * cus + 5


STAGE_SHAPES = [(3, 51), (6, 51), (2, 2), (5, 33), (17, 64)]
SUPPORTS = [(0.0, 200.0, 51), (-3.5, 1.25, 7), (-1.0, 1.0, 2), (-1000.0, 1000.0, 64)]
GAMMAS = [0.0, 1.0, GAMMA]
SHARD = dict(B=4, A=3, N=51, dueling=1, seed=5)
MI355X_CUS = 256


def families(cus=MI355X_CUS):
    """name -> family() keywords of every input the GPU edge tests launch"""
    f = {}
    for A, N in STAGE_SHAPES:
        for dueling in (1, 0):
            f[f'stage-{A}x{N}-d{dueling}'] = dict(B=9, A=A, N=N, dueling=dueling, seed=A + N)
    for dueling in (1, 0):
        f[f'lds-48x64-d{dueling}'] = dict(B=5, A=48, N=64, dueling=dueling, seed=48)
    for B in row_block_sizes(cus):
        f[f'blocks-{B}'] = dict(B=B, A=2, N=3, dueling=1, seed=1)
    f['shard'] = dict(SHARD)
    for v_min, v_max, N in SUPPORTS:
        for gamma in GAMMAS:
            f[f'corner-{v_min:g}_{v_max:g}x{N}-g{gamma:.2f}'] = dict(
                B=9, A=3, N=N, dueling=int(N != 7), v_min=v_min, v_max=v_max, gamma=gamma, seed=N,
                done_half=True, inf=True)
    return f


def params(kw):
    """(A, N, v_min, v_max, gamma) of a family's keywords"""
    return kw['A'], kw['N'], kw.get('v_min', -10.0), kw.get('v_max', 10.0), kw.get('gamma', GAMMA)


def refs_of(c, kw, double_q, weighted, B_global=None):
    """(c51_td in float32 with autograd's dadv / dval, the same in float64, c51_td_loop) on the
    inputs c of a family with keywords kw; B_global: the shard forms' divisor"""
    (A, N, v_min, v_max, gamma), B_global = params(kw), B_global or kw['B']
    w = c['w'] if weighted else None
    r = {}
    for dt in (torch.float32, torch.float64):
        cv = lambda pr: tuple(None if t is None else t.to(dt) for t in pr)             # noqa: E731
        online = tuple(None if t is None else t.clone().requires_grad_() for t in cv(c['q']))
        out = c51_td(online, cv(c['n']) if double_q else None, cv(c['t']), c['act'], c['rew'], c['done'],
                     w, A, N, v_min, v_max, gamma)
        (out['objective'] * (kw['B'] / B_global)).backward()
        out['stats'] = out['stats'] * (kw['B'] / B_global)
        out['dadv'], out['dval'] = online[0].grad, None if online[1] is None else online[1].grad
        r[dt] = out
    loop = c51_td_loop(c['q'], c['n'] if double_q else None, c['t'], c['act'], c['rew'], c['done'], w,
                       A, N, v_min, v_max, gamma, B_global)
    return r[torch.float32], r[torch.float64], loop


@functools.lru_cache(maxsize=None)
def _refs(key, double_q, weighted, B_global):
    kw = dict(key)
    return refs_of(family(**kw), kw, double_q, weighted, B_global)


def refs(kw, double_q, weighted, B_global=None):
    """refs_of on the family's own inputs; cached, so the results are shared: read-only"""
    return _refs(tuple(sorted(kw.items())), bool(double_q), bool(weighted), B_global or kw['B'])
