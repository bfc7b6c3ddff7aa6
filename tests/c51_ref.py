"""Categorical (C51) DQN in plain torch on the CPU, dtype-generic: the textbook floor / ceil
index_add_ projection and log_softmax, deliberately not the gather form of dqn_dist_kernels.hip."""
import torch
import torch.nn as nn

from tests.dqn_ref import FFQfuncRef


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
        b = (((r + gamma * ((1 - d) * z)).clamp(v_min, v_max) - v_min) / delta).clamp(0, N - 1)
        lo, up = b.floor(), b.ceil()
        off = (rows * N)[:, None]
        m = torch.zeros(B * N, dtype=dt)
        m.index_add_(0, (lo.long() + off).reshape(-1), (pt * ((up - b) + (lo == up).to(dt))).reshape(-1))
        m.index_add_(0, (up.long() + off).reshape(-1), (pt * (b - lo)).reshape(-1))
        m = m.view(B, N)
    logp = torch.log_softmax(logits(*online, A, N), 2)[rows, actions.reshape(B).long()]
    td = -(m * logp).sum(1)
    wv = torch.ones(B, dtype=dt) if w is None else w.reshape(B).to(dt)
    return {'q_sel': q_sel, 'astar': astar, 'm': m, 'td': td.detach(), 'objective': (wv * td).sum() / B,
            'stats': torch.stack([(wv * td).sum() / B, td.sum() / B]).detach()}
