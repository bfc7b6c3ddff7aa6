"""Quantile-regression DQN reference on the CPU: plain torch, dtype-generic, the
pairs materialised as u [B][N][N] and the Huber branches by torch.where;
gradients come from autograd (nothing flows through the indicator or T)."""
import torch
import torch.nn as nn

from tests.c51_ref import action_index
from tests.dqn_ref import FFQfuncRef


def twin(D, A, N, hidden, dueling):
    """FFQfuncRef with quantile heads: streams(x) = (adv [B][A N], val [B][N] | None)"""
    net = FFQfuncRef(D, A * N, hidden, dueling)
    if dueling:
        net.fc_state_layers[-1] = nn.Linear(hidden[-1], N)
    return net


def quantiles(adv, val, A, N):
    th = adv.reshape(-1, A, N)
    return th if val is None else (th - th.mean(dim=1, keepdim=True)) + val[:, None, :]


def mean_q(adv, val, A, N):
    return quantiles(adv, val, A, N).mean(2)


def qr_td(online, nxt, target, actions, rewards, dones, w, A, N, kappa, gamma):
    """online / nxt (None without double-Q) / target: (adv, val | None) at s, s', s'.
    q_sel is the selecting net's Q(s'), T [B][N] the targets, td the row losses,
    objective mean(w td), stats (mean(w td), mean(td)); u [B][i][j] = T_j - theta_i."""
    dt = online[0].dtype
    B, rows = online[0].shape[0], torch.arange(online[0].shape[0])
    with torch.no_grad():
        q_sel = mean_q(*(nxt or target), A, N)
        astar = q_sel.argmax(1)                                 # the first maximum
        r, d = rewards.reshape(B, 1).to(dt), dones.reshape(B, 1).to(dt)
        T = r + gamma * ((1 - d) * quantiles(*target, A, N)[rows, astar])
    theta = quantiles(*online, A, N)[rows, action_index(actions, A)]
    tau = (2 * torch.arange(N, dtype=dt) + 1) / (2 * N)
    u = T[:, None, :] - theta[:, :, None]
    au = u.abs()
    if kappa > 0:
        L = torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
    else:
        L = au
    rho = (tau[None, :, None] - (u.detach() < 0).to(dt)).abs() * L
    td = rho.sum(1).mean(1)
    wv = torch.ones(B, dtype=dt) if w is None else w.reshape(B).to(dt)
    objective = (wv * td).sum() / B
    return {'q_sel': q_sel, 'astar': astar, 'T': T, 'u': u.detach(), 'td': td.detach(),
            'objective': objective, 'stats': torch.stack([objective.detach(), td.detach().mean()])}
