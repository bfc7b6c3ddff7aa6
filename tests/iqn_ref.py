"""Implicit quantile DQN reference on the CPU: plain torch, dtype-generic, the
cosine features by torch.cos, the pairs materialised as u [B][N][N'] and the
gradients by autograd (nothing flows through the indicator or T); the
fractions of smi_iqn_taus by a numpy Philox4x32-10."""
import math

import numpy as np
import torch
import torch.nn as nn

from tests.c51_ref import action_index
from tests.dqn_ref import FFQfuncRef
from tests.qconv_ref import QConvRef


def philox(key, ctr):
    """Philox4x32-10: key (2,) uint32, ctr (n, 4) uint32 -> (n, 4) uint32"""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    k0, k1 = int(key[0]), int(key[1])
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    lo32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def taus(seed, step, stream_id, row0, rows, N):
    """smi_iqn_taus: float32 [rows * N]"""
    g = np.arange(row0 * N, (row0 + rows) * N, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full_like(g, step),
                    np.full_like(g, stream_id)], 1)
    x = philox((seed & 0xFFFFFFFF, seed >> 32), ctr)[:, 0]
    return (((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23).astype(np.float32)


def embed(tau, H1, weight, bias, N):
    """(Z, phi) [B N][d] of tau [B N], H1 [B][d], weight [d][n_cos], bias [d]"""
    i = torch.arange(weight.shape[1], dtype=tau.dtype)
    phi = torch.relu(torch.cos(math.pi * i[None, :] * tau[:, None]) @ weight.t() + bias)
    return H1.repeat_interleave(N, 0) * phi, phi


def twin(D, A, hidden, dueling, n_cos, pixel=None):
    """FFQfuncRef (pixel = (input_shape, convs): QConvRef on uint8 frames) plus
    fc_tau_layer, the last entry of its state_dict"""
    net = FFQfuncRef(D, A, hidden, dueling) if pixel is None else \
        QConvRef(pixel[0], A, pixel[1], hidden, dueling, True)
    net.fc_tau_layer = nn.Linear(n_cos, (2 if dueling else 1) * hidden[0])
    return net


def streams(net, x, tau, N):
    """(adv [B N][A], val [B N][1] | None) of the twin at the fractions tau [B N]"""
    if hasattr(net, 'features'):
        x = net.features(x)
    nets = [net.fc_action_layers] + ([net.fc_state_layers] if net.dueling else [])
    H1 = torch.cat([torch.relu(layers[0](x)) for layers in nets], 1)
    Z = embed(tau, H1, net.fc_tau_layer.weight, net.fc_tau_layer.bias, N)[0]
    outs = []
    for h, layers in zip(Z.chunk(len(nets), 1), nets):
        for k in range(1, len(layers)):
            h = layers[k](h)
            h = torch.relu(h) if k < len(layers) - 1 else h
        outs.append(h)
    return outs[0], (outs[1] if net.dueling else None)


def theta(adv, val, A, n):
    th = adv.reshape(-1, n, A)
    return th if val is None else (th - th.mean(dim=2, keepdim=True)) + val.reshape(-1, n, 1)


def mean_q(adv, val, A, n):
    return theta(adv, val, A, n).mean(1)


def iqn_td(online, nxt, target, tau, actions, rewards, dones, w, A, N, Nt, kappa, gamma):
    """online (N samples, fractions tau [B N]) / nxt (None without double-Q) /
    target (Nt samples): (adv, val | None).  q_sel is the selecting net's Q(s'),
    T [B][Nt] the targets, td the row losses, objective mean(w td), stats
    (mean(w td), mean(td)); u [B][i][j] = T_j - theta_i."""
    dt = online[0].dtype
    B = online[0].shape[0] // N
    rows = torch.arange(B)
    with torch.no_grad():
        q_sel = mean_q(*(nxt or target), A, Nt)
        astar = q_sel.argmax(1)                                 # the first maximum
        r, d = rewards.reshape(B, 1).to(dt), dones.reshape(B, 1).to(dt)
        T = r + gamma * ((1 - d) * theta(*target, A, Nt)[rows, :, astar])
    th = theta(*online, A, N)[rows, :, action_index(actions, A)]
    u = T[:, None, :] - th[:, :, None]
    au = u.abs()
    if kappa > 0:
        L = torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
    else:
        L = au
    rho = (tau.reshape(B, N, 1).to(dt) - (u.detach() < 0).to(dt)).abs() * L
    td = rho.sum(1).mean(1)
    wv = torch.ones(B, dtype=dt) if w is None else w.reshape(B).to(dt)
    objective = (wv * td).sum() / B
    return {'q_sel': q_sel, 'astar': astar, 'T': T, 'u': u.detach(), 'td': td.detach(),
            'objective': objective, 'stats': torch.stack([objective.detach(), td.detach().mean()])}
