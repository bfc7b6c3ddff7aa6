"""Times one DQNLearner.learn() (dueling double-Q, B = 512, D = 17, hidden
[128, 128], A = 6, importance weights) eagerly and as a hipGraph replay, and in
the same process DDPGLearner.learn() at the C4 shape (batch 512, 17 -> 6,
actor 300x200, critic 400x300) as the yardstick: HIP events around each call,
median of --iters calls after warm-up (as tools/bench_hbm.py).  The launch count
of a DQN step is taken from the library calls of one eager step (a grouped
weight-gradient flush is two launches, smi_adam_clip with a norm clip three;
queued weight gradients and smi_dw_group_begin launch nothing).  Prints one
JSON line per measurement; reads nothing outside the repository.

--pixel times the Atari-shaped step instead: 4x84x84 uint8 frames, convs
[[32, 8, 4], [64, 4, 2], [64, 3, 1]], hidden [512], A = 6, at B = 32 and
B = 512, eager and as a graph replay, and next to each the same step written in
eager torch on the same GPU (nn.Conv2d through MIOpen, fp32, Adam eps 1e-4,
clip_grad_norm_ 10): the expectation a pixel learn() is reported against.  When
the torch step cannot run, that is printed and the project's numbers stand alone.
--conv-bf16 adds the same step with model.conv_dtype = 'bf16' to each.

--gpus N (2 <= N <= 16) times the data-parallel loop instead: one process per
GPU (torch.multiprocessing spawn, 'nccl' = RCCL), each with one
DQNLearner(dp=TorchDistAllReduce()) and one PrioritizedReplay replica, a step
being sample_shard -> learn -> update_priorities_from_td at a global batch of
512 (512 / N rows per rank).  Rank 0 prints the one JSON line.  With fewer than
N (or fewer than two) GPUs visible it says so and starts nothing.

--atoms N (2 <= N <= 64) times the categorical (C51) head instead: learn()
with algo.distributional.enabled next to the scalar learner's, eager and as a
graph replay, and at B = 512 and A in {6, 18} (dueling, double-Q, weights) one
smi_dqn_c51_td call (the TD kernel and its statistics launch) next to the same
math in eager torch on the same GPU tensors (log_softmax, index_add_
projection, autograd to the three head outputs): what a user would otherwise
write.  Each timed sample is --calls back-to-back calls between two events.

--quantiles N [--kappa K] (1 <= N <= 256) does the same for the quantile head
(QR-DQN): one smi_dqn_qr_td call next to the same math in eager torch (the
pairs as u [B][N][N], torch.where for the Huber branches, autograd to the head
outputs), and learn() with algo.distributional.kind = 'quantile' next to the
scalar learner's.

--implicit [--atoms N] (1 <= N <= 64, default 8) times the implicit quantile
head (IQN) at B = 512, N = N' samples, d = 256 and 64 cosines: one
smi_iqn_embed_forward and one smi_iqn_embed_backward call with the bytes per
second of what each must read and write once, one smi_iqn_td call at A in
{6, 18}, and learn() with algo.distributional.kind = 'implicit', eager and as
a graph replay.

--fc-bf16 times model.fc_dtype = 'bf16' against 'fp32', the two arms alternating
call by call in one process: smi_linear_forward and smi_linear_backward_input
against their _bf16 twins at the FC shapes of the DQN models (512 rows, and the
32768 sample rows of implicit heads at B = 512, N = 64), then learn() at the
Atari shape (B = 32 and 512, conv_dtype 'bf16' on both arms) and of the
low-dimensional model with implicit heads (B = 512, 64 samples), eager and as a
graph replay.

--fc-bf16-all times model.fc_dtype = 'bf16_all' against 'bf16' the same way:
smi_linear_backward_weight against smi_linear_backward_weight_bf16 at those
shapes, one call each (the small 512-row layers also as one grouped fp32 launch
against three bf16 calls), then the same learn() cases with 'bf16' and 'bf16_all'.

--noisy --noisy-bf16 / --noisy-bf16-all time model.noisy.dtype = 'bf16' /
'bf16_all' against 'fp32', the two arms alternating: smi_noisy_forward and
smi_noisy_backward_input against their _bf16 twins at the shapes of --fc-bf16,
then --noisy's learn() (with --pixel, --implicit, .. as there) on the two values.

Usage: python tools/bench_dqn.py [--iters 40] [--warmup 10]
                                 [--pixel [--conv-bf16] | --gpus N | --atoms N | --quantiles N [--kappa K]
                                  | --implicit [--atoms N] | --fc-bf16 | --fc-bf16-all
                                  | --noisy [--noisy-bf16 | --noisy-bf16-all]]
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from surreal_amd import _lib as L  # noqa: E402
from surreal_amd import synthetic  # noqa: E402
from surreal_amd.config import (DDPG_DEFAULT_LEARNER_CONFIG, DQN_DEFAULT_LEARNER_CONFIG,  # noqa: E402
                                discrete_env_config, discrete_pixel_env_config, gym_env_config)
from surreal_amd.ddpg import DDPGLearner  # noqa: E402
from surreal_amd.dqn import DQNLearner  # noqa: E402

LAUNCHES = {'smi_dw_group_begin': 0, 'smi_linear_backward_weight': 0, 'smi_dw_group_flush': 2,
            'smi_adam_clip': 3}


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    return ts[len(ts) // 2], ts[len(ts) // 4], ts[3 * len(ts) // 4]


def timed_alternating(fns, iters, warm):
    """timed() of several arms, one call of each per round: [(median, q1, q3)]"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    evs = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            evs[i].append((s, e))
    torch.cuda.synchronize()
    out = []
    for ev in evs:
        ts = sorted(s.elapsed_time(e) for s, e in ev)
        out.append((ts[len(ts) // 2], ts[len(ts) // 4], ts[3 * len(ts) // 4]))
    return out


def count_launches(fn):
    calls, real = [], L.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)
    L.call = counting
    try:
        fn()
    finally:
        L.call = real
    return sum(LAUNCHES.get(n, 1) for n in calls), len(calls)


def dqn_batch(B, D, A, seed):
    g = torch.Generator().manual_seed(seed)
    return {'obs': torch.randn(B, D, generator=g).cuda(),
            'actions': torch.randint(0, A, (B, 1), generator=g).float().cuda(),
            'rewards': torch.randn(B, 1, generator=g).cuda(),
            'obs_next': torch.randn(B, D, generator=g).cuda(),
            'dones': (torch.rand(B, 1, generator=g) < 0.05).float().cuda(),
            'weights': (0.3 + 0.7 * torch.rand(B, 1, generator=g)).cuda()}


NATURE = [[32, 8, 4], [64, 4, 2], [64, 3, 1]]


def pixel_batch(B, shape, A, seed):
    g = torch.Generator().manual_seed(seed)
    return {'obs': torch.randint(0, 256, (B,) + shape, generator=g, dtype=torch.uint8).cuda(),
            'actions': torch.randint(0, A, (B, 1), generator=g).float().cuda(),
            'rewards': torch.randn(B, 1, generator=g).cuda(),
            'obs_next': torch.randint(0, 256, (B,) + shape, generator=g, dtype=torch.uint8).cuda(),
            'dones': (torch.rand(B, 1, generator=g) < 0.05).float().cuda(),
            'weights': (0.3 + 0.7 * torch.rand(B, 1, generator=g)).cuda()}


class TorchQ(torch.nn.Module):
    """q_net.py:68-119 in plain torch (dueling, is_uint8)"""

    def __init__(self, shape, A, hidden):
        super().__init__()
        nn, c, hw = torch.nn, shape[0], shape[1]
        convs = []
        for co, k, s in NATURE:
            convs += [nn.Conv2d(c, co, k, stride=s, padding=k // 2), nn.ReLU()]
            c, hw = co, (hw + 2 * (k // 2) - k) // s + 1
        self.stem = nn.Sequential(*convs, nn.Flatten())
        F = c * hw * hw
        self.adv = nn.Sequential(nn.Linear(F, hidden), nn.ReLU(), nn.Linear(hidden, A))
        self.val = nn.Sequential(nn.Linear(F, hidden), nn.ReLU(), nn.Linear(hidden, 1))

    def forward(self, x):
        f = self.stem(x / 255.0)
        a = self.adv(f)
        return a - a.mean(1, keepdim=True) + self.val(f)


def torch_step(q, qt, opt, b, gamma=0.99):
    """dqn.py:42-73 (double-Q, Huber, importance weights, norm clip 10)"""
    a = b['actions'].long()
    qa = q(b['obs']).gather(1, a)
    with torch.no_grad():
        best = q(b['obs_next']).max(1, keepdim=True)[1]
        y = b['rewards'] + gamma * (1.0 - b['dones']) * qt(b['obs_next']).gather(1, best)
    td = qa - y
    loss = (b['weights'] * torch.where(td.abs() < 1.0, 0.5 * td * td, td.abs() - 0.5)).mean()
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(q.parameters(), 10)
    opt.step()


def pixel_main(args):
    shape, A, hidden = (4, 84, 84), 6, 512
    ec = discrete_pixel_env_config(shape, A)
    for B in (32, 512):
        lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
        lc.replay.batch_size = B
        lc.model.convs, lc.model.fc_hidden_sizes = NATURE, [hidden]
        b = pixel_batch(B, shape, A, 0)
        runs = [('dqn_pixel_learn_eager', False, 'fp32'), ('dqn_pixel_learn_graph', True, 'fp32')]
        if args.conv_bf16:
            runs += [('dqn_pixel_learn_eager', False, 'bf16'), ('dqn_pixel_learn_graph', True, 'bf16')]
        for name, graph, conv_dtype in runs:
            lc.model.conv_dtype = conv_dtype
            learner = DQNLearner(lc, ec, seed=0, use_graph=graph)
            extra = {'conv_dtype': conv_dtype}
            if not graph:
                learner.learn(b)
                extra['library_calls_per_step'] = count_launches(lambda: learner.learn(b))[1]
            med, q1, q3 = timed(lambda: learner.learn(b), args.iters, args.warmup)
            print(json.dumps(dict({'measurement': name, 'B': B, 'median_ms': round(med, 4),
                                   'q1_ms': round(q1, 4), 'q3_ms': round(q3, 4),
                                   'iters': args.iters}, **extra)), flush=True)
            del learner
        try:
            torch.manual_seed(0)
            q, qt = TorchQ(shape, A, hidden).cuda(), TorchQ(shape, A, hidden).cuda()
            opt = torch.optim.Adam(q.parameters(), lr=1e-3, eps=1e-4)
            med, q1, q3 = timed(lambda: torch_step(q, qt, opt, b), args.iters, args.warmup)
            print(json.dumps({'measurement': 'torch_eager_pixel_step', 'B': B,
                              'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                              'q3_ms': round(q3, 4), 'iters': args.iters}), flush=True)
        except RuntimeError as e:
            print(json.dumps({'measurement': 'torch_eager_pixel_step', 'B': B,
                              'not_measured': str(e).splitlines()[0][:200]}), flush=True)


def dp_worker(rank, world, port, iters, warmup):
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    import torch.distributed as dist
    from surreal_amd.learner import TorchDistAllReduce
    from surreal_amd.replay import PrioritizedReplay
    torch.cuda.set_device(rank)
    dev = f'cuda:{rank}'
    dist.init_process_group('nccl', rank=rank, world_size=world)
    Bg, D, A, rows = 512, 17, 6, 20000
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = Bg // world
    lc.replay.memory_size, lc.replay.sampling_start_size = rows, 1000
    lc.model.fc_hidden_sizes = [128, 128]
    ec = discrete_env_config(D, A)
    replay = PrioritizedReplay(lc, ec, seed=0, device=dev)
    g = torch.Generator().manual_seed(0)
    table = torch.randn(rows, 2 * D + 3, generator=g)
    table[:, D] = torch.randint(0, A, (rows,), generator=g).float()
    table[:, 2 * D + 2] = (torch.rand(rows, generator=g) < 0.05).float()
    replay.insert_rows(table)
    learner = DQNLearner(lc, ec, seed=0, device=dev, dp=TorchDistAllReduce())

    def step():
        idx_all, batch = replay.sample_shard(Bg, rank, world, beta=0.4)
        learner.learn(batch)
        replay.update_priorities_from_td(idx_all, learner.td_error)
    med, q1, q3 = timed(step, iters, warmup)
    if rank == 0:
        print(json.dumps({'measurement': 'dqn_dp_per_loop', 'gpus': world, 'B_global': Bg,
                          'backend': 'nccl', 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                          'q3_ms': round(q3, 4), 'iters': iters}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def dp_main(args):
    import socket
    import torch.multiprocessing as mp
    n, seen = args.gpus, torch.cuda.device_count()
    if not 2 <= n <= 16 or 512 % n:
        sys.exit(f'--gpus {n}: takes 2 to 16 processes that divide the batch of 512')
    if seen < 2 or seen < n:
        sys.exit(f'--gpus {n}: {seen} GPU(s) visible, nothing started')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(dp_worker, args=(n, port, args.iters, args.warmup), nprocs=n, join=True)


def torch_c51(adv, val, adv_n, val_n, adv_t, val_t, act, rew, done, w, A, N, v_min, v_max, gamma):
    """the categorical TD step in eager torch: dueling logits, double-Q arg-max
    of the expected values, floor / ceil projection, weighted cross-entropy and
    its gradients at (adv, val)"""
    B = adv.shape[0]
    lg = lambda a, v: (lambda l: (l - l.mean(1, keepdim=True)) + v[:, None, :])(a.view(B, A, N))  # noqa: E731
    delta = (v_max - v_min) / (N - 1)
    z = v_min + torch.arange(N, device=adv.device, dtype=adv.dtype) * delta
    rows = torch.arange(B, device=adv.device)
    with torch.no_grad():
        astar = (torch.softmax(lg(adv_n, val_n), 2) * z).sum(2).argmax(1)
        pt = torch.softmax(lg(adv_t, val_t), 2)[rows, astar]
        b = ((rew + gamma * ((1 - done) * z)).clamp(v_min, v_max) - v_min) / delta
        lo, up = b.floor(), b.ceil()
        off = (rows * N)[:, None]
        m = torch.zeros(B * N, device=adv.device)
        m.index_add_(0, (lo.long() + off).view(-1), (pt * ((up - b) + (lo == up).float())).view(-1))
        m.index_add_(0, (up.long() + off).view(-1), (pt * (b - lo)).view(-1))
    logp = torch.log_softmax(lg(adv, val), 2)[rows, act]
    loss = -(m.view(B, N) * logp).sum(1)
    return torch.autograd.grad((w * loss).mean(), (adv, val)), loss.detach()


def torch_qr(adv, val, adv_n, val_n, adv_t, val_t, act, rew, done, w, A, N, kappa, gamma):
    """the quantile TD step in eager torch: dueling quantiles, double-Q arg-max of
    their means, every (online, target) pair, the weighted quantile-Huber loss
    and its gradients at (adv, val)"""
    B = adv.shape[0]
    th = lambda a, v: (lambda l: (l - l.mean(1, keepdim=True)) + v[:, None, :])(a.view(B, A, N))  # noqa: E731
    rows = torch.arange(B, device=adv.device)
    with torch.no_grad():
        astar = th(adv_n, val_n).mean(2).argmax(1)
        T = rew + gamma * ((1 - done) * th(adv_t, val_t)[rows, astar])
    tau = (2 * torch.arange(N, device=adv.device, dtype=adv.dtype) + 1) / (2 * N)
    u = T[:, None, :] - th(adv, val)[rows, act][:, :, None]
    au = u.abs()
    hub = torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa if kappa > 0 else au
    loss = ((tau[None, :, None] - (u.detach() < 0).float()).abs() * hub).sum(1).mean(1)
    return torch.autograd.grad((w * loss).mean(), (adv, val)), loss.detach()


def dist_main(args):
    """--atoms N (the categorical head) or --quantiles N (the quantile head)"""
    quant = bool(args.quantiles)
    N, B, D, v_min, v_max, gamma = args.quantiles or args.atoms, 512, 17, -10.0, 10.0, 0.99
    key = 'quantiles' if quant else 'atoms'
    p, st = L.ptr, L.stream()
    for A in (6, 18):
        g = torch.Generator().manual_seed(A)
        adv, adv_n, adv_t = (torch.randn(B, A * N, generator=g).cuda() for _ in range(3))
        val, val_n, val_t = (torch.randn(B, N, generator=g).cuda() for _ in range(3))
        b = dqn_batch(B, D, A, 0)
        act, rew, done, w = b['actions'], b['rewards'], b['dones'], b['weights']
        dadv, dval, td = torch.zeros(B, A * N).cuda(), torch.zeros(B, N).cuda(), torch.zeros(B).cuda()
        stats = torch.zeros(2).cuda()
        need = int((L.lib().smi_dqn_qr_partials_bytes if quant else L.lib().smi_dqn_c51_partials_bytes)(B))
        part = torch.zeros(need // 8, dtype=torch.float64).cuda()

        def hip_qr():
            for _ in range(args.calls):
                L.call('smi_dqn_qr_td', p(adv), A * N, p(adv_n), A * N, p(adv_t), A * N, p(val), N,
                       p(val_n), N, p(val_t), N, p(act), 1, p(rew), 1, p(done), 1, p(w), B, A, N,
                       args.kappa, gamma, 1, 1, p(dadv), A * N, p(dval), N, p(td), None, None, p(part),
                       need, p(stats), st)

        def hip():
            for _ in range(args.calls):
                L.call('smi_dqn_c51_td', p(adv), A * N, p(adv_n), A * N, p(adv_t), A * N, p(val), N,
                       p(val_n), N, p(val_t), N, p(act), 1, p(rew), 1, p(done), 1, p(w), B, A, N, v_min,
                       v_max, gamma, 1, 1, p(dadv), A * N, p(dval), N, p(td), None, None, p(part),
                       need, p(stats), st)
        ga, gv = adv.clone().requires_grad_(), val.clone().requires_grad_()

        def eager():
            for _ in range(args.calls):
                torch_c51(ga, gv, adv_n, val_n, adv_t, val_t, act.view(B).long(), rew, done,
                          w.view(B), A, N, v_min, v_max, gamma)

        def eager_qr():
            for _ in range(args.calls):
                torch_qr(ga, gv, adv_n, val_n, adv_t, val_t, act.view(B).long(), rew, done,
                         w.view(B), A, N, args.kappa, gamma)
        for name, fn in ((('qr_td_and_stats', hip_qr), ('torch_eager_qr_td', eager_qr)) if quant else
                         (('c51_td_and_stats', hip), ('torch_eager_c51_td', eager))):
            med, q1, q3 = (1e3 * t / args.calls for t in timed(fn, args.iters, args.warmup))
            print(json.dumps({'measurement': name, 'B': B, 'A': A, key: N,
                              'median_us_per_call': round(med, 2), 'q1_us': round(q1, 2),
                              'q3_us': round(q3, 2), 'calls_per_sample': args.calls,
                              'iters': args.iters}), flush=True)
    A = 6
    b = dqn_batch(B, D, A, 0)
    for atoms in (None, N):
        lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
        lc.replay.batch_size = B
        lc.algo.distributional.enabled, lc.algo.distributional.atoms = atoms is not None, N
        if quant:
            lc.algo.distributional.kind, lc.algo.distributional.kappa = 'quantile', args.kappa
        for graph in (False, True):
            learner = DQNLearner(lc, discrete_env_config(D, A), seed=0, use_graph=graph)
            med, q1, q3 = timed(lambda: learner.learn(b), args.iters, args.warmup)
            print(json.dumps({'measurement': 'dqn_learn_' + ('graph' if graph else 'eager'),
                              key: atoms, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                              'q3_ms': round(q3, 4), 'iters': args.iters}), flush=True)


def implicit_main(args):
    """--implicit [--atoms N]: the implicit quantile (IQN) kernels at B = 512, N = N' samples,
    d = 256, 64 cosines (bytes: what each launch must read and write once), and learn()"""
    N, B, D, d, n_cos, gamma = args.atoms or 8, 512, 17, 256, 64, 0.99
    p, st, M = L.ptr, L.stream(), 512 * (args.atoms or 8)
    g = torch.Generator().manual_seed(N)
    tau = torch.rand(M, generator=g).cuda()
    H1, W, bias = torch.rand(B, d, generator=g).cuda(), (torch.randn(d, n_cos, generator=g) / 8).cuda(), \
        torch.zeros(d).cuda()
    Z, phi, dZ, dH1 = torch.zeros(M, d).cuda(), torch.zeros(M, d).cuda(), torch.randn(M, d, generator=g).cuda(), \
        torch.zeros(B, d).cuda()
    dW, db = torch.zeros(d, n_cos).cuda(), torch.zeros(d).cuda()
    need = int(L.lib().smi_iqn_embed_scratch_bytes(B, N, n_cos, d))
    scratch = torch.zeros(max(need // 4, 1)).cuda()

    def fwd():
        for _ in range(args.calls):
            L.call('smi_iqn_embed_forward', p(tau), p(H1), d, B, N, p(W), p(bias), n_cos, d, p(Z), d,
                   p(phi), d, st)

    def bwd():
        for _ in range(args.calls):
            L.call('smi_iqn_embed_backward', p(dZ), d, p(tau), p(H1), d, p(phi), d, B, N, p(dW), p(db),
                   n_cos, d, p(dH1), d, p(scratch), need, st)
    # forward: Z and phi out, H1 in; backward: dZ and phi in twice (dH1, dW), H1 in, dH1 out
    for name, fn, nbytes in (('iqn_embed_forward', fwd, 4 * (2 * M * d + B * d)),
                             ('iqn_embed_backward', bwd, 4 * (4 * M * d + 3 * B * d))):
        med, q1, q3 = (1e3 * t / args.calls for t in timed(fn, args.iters, args.warmup))
        print(json.dumps({'measurement': name, 'B': B, 'atoms': N, 'd': d, 'n_cos': n_cos,
                          'median_us_per_call': round(med, 2), 'q1_us': round(q1, 2),
                          'q3_us': round(q3, 2), 'GB_per_s': round(nbytes / med / 1e3, 1),
                          'calls_per_sample': args.calls, 'iters': args.iters}), flush=True)
    for A in (6, 18):
        adv, adv_n, adv_t = (torch.randn(M, A, generator=g).cuda() for _ in range(3))
        val, val_n, val_t = (torch.randn(M, generator=g).cuda() for _ in range(3))
        b = dqn_batch(B, D, A, 0)
        act, rew, done, w = b['actions'], b['rewards'], b['dones'], b['weights']
        dadv, dval, td, stats = torch.zeros(M, A).cuda(), torch.zeros(M).cuda(), torch.zeros(B).cuda(), \
            torch.zeros(2).cuda()
        pneed = int(L.lib().smi_iqn_partials_bytes(B))
        part = torch.zeros(pneed // 8, dtype=torch.float64).cuda()

        def td_call():
            for _ in range(args.calls):
                L.call('smi_iqn_td', p(adv), A, p(adv_n), A, p(adv_t), A, p(val), p(val_n), p(val_t),
                       p(tau), p(act), 1, p(rew), 1, p(done), 1, p(w), B, A, N, N, args.kappa, gamma, 1, 1,
                       p(dadv), A, p(dval), p(td), None, None, p(part), pneed, p(stats), st)
        med, q1, q3 = (1e3 * t / args.calls for t in timed(td_call, args.iters, args.warmup))
        print(json.dumps({'measurement': 'iqn_td_and_stats', 'B': B, 'A': A, 'atoms': N,
                          'median_us_per_call': round(med, 2), 'q1_us': round(q1, 2),
                          'q3_us': round(q3, 2), 'calls_per_sample': args.calls,
                          'iters': args.iters}), flush=True)
    A = 6
    b = dqn_batch(B, D, A, 0)
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    lc.model.fc_hidden_sizes = [128, 128]
    lc.algo.distributional.update(enabled=True, kind='implicit', atoms=N, kappa=args.kappa)
    for graph in (False, True):
        learner = DQNLearner(lc, discrete_env_config(D, A), seed=0, use_graph=graph)
        med, q1, q3 = timed(lambda: learner.learn(b), args.iters, args.warmup)
        print(json.dumps({'measurement': 'dqn_learn_' + ('graph' if graph else 'eager'),
                          'implicit_atoms': N, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                          'q3_ms': round(q3, 4), 'iters': args.iters}), flush=True)


def noisy_main(args):
    """--noisy [--pixel] [--atoms N | --quantiles N | --implicit]: learn() at B = 512 with the
    plain and the noisy layers, eager and replayed, and the noisy forward against
    smi_linear_forward at the FC shapes of the low-dim default and of the pixel model"""
    B, D, A = 512, 17, 6
    p, st = L.ptr, L.stream()
    dtype = 'bf16_all' if args.noisy_bf16_all else 'bf16' if args.noisy_bf16 else None
    if dtype:
        noisy_bf16_layers(args)
    g = torch.Generator().manual_seed(0)
    for K, N in () if dtype else ((17, 256), (128, 128), (128, 6), (3136, 1024), (512, 6)):
        x, y = torch.randn(B, K, generator=g).cuda(), torch.zeros(B, N).cuda()
        w, ws, b, bs = (torch.randn(*sh, generator=g).cuda() / K ** 0.5 for sh in ((N, K), (N, K), (N,), (N,)))
        fi, fo = torch.randn(K, generator=g).cuda(), torch.randn(N, generator=g).cuda()

        def plain():
            for _ in range(args.calls):
                L.call('smi_linear_forward', p(x), K, B, K, p(w), K, p(b), N, 1, p(y), N, st)

        def noisy():
            for _ in range(args.calls):
                L.call('smi_noisy_forward', p(x), K, B, K, p(w), p(ws), K, p(b), p(bs), p(fi), p(fo), N, 1,
                       p(y), N, st)
        for name, fn in (('linear_forward', plain), ('noisy_forward', noisy)):
            med, q1, q3 = (1e3 * t / args.calls for t in timed(fn, args.iters, args.warmup))
            print(json.dumps({'measurement': name, 'rows': B, 'in': K, 'out': N,
                              'median_us_per_call': round(med, 2), 'q1_us': round(q1, 2),
                              'q3_us': round(q3, 2), 'calls_per_sample': args.calls,
                              'iters': args.iters}), flush=True)
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    lc.model.fc_hidden_sizes = [128, 128]
    ec, b = discrete_env_config(D, A), None
    if args.pixel:
        shape = (4, 84, 84)
        lc.model.convs, lc.model.fc_hidden_sizes = NATURE, [512]
        ec, b = discrete_pixel_env_config(shape, A), pixel_batch(B, shape, A, 0)
    b = b if b is not None else dqn_batch(B, D, A, 0)
    if args.implicit:
        lc.algo.distributional.update(enabled=True, kind='implicit', atoms=args.atoms or 8)
    elif args.quantiles:
        lc.algo.distributional.update(enabled=True, kind='quantile', atoms=args.quantiles, kappa=args.kappa)
    elif args.atoms:
        lc.algo.distributional.update(enabled=True, atoms=args.atoms)
    for graph in (False, True) if dtype else ():      # the noisy step on 'fp32' and on dtype, alternating
        learners = []
        for arm in ('fp32', dtype):
            lc.model.noisy.update(enabled=True, dtype=arm)
            learners.append(DQNLearner(lc, ec, seed=0, use_graph=graph))
        res = timed_alternating([lambda ln=ln: ln.learn(b) for ln in learners], args.iters, args.warmup)
        for arm, (med, q1, q3) in zip(('fp32', dtype), res):
            print(json.dumps({'measurement': 'dqn_learn_' + ('graph' if graph else 'eager'), 'noisy': True,
                              'noisy_dtype': arm, 'pixel': bool(args.pixel), 'median_ms': round(med, 4),
                              'q1_ms': round(q1, 4), 'q3_ms': round(q3, 4), 'iters': args.iters}), flush=True)
        del learners
    for noisy_on in () if dtype else (False, True):
        lc.model.noisy.enabled = noisy_on
        for graph in (False, True):
            learner = DQNLearner(lc, ec, seed=0, use_graph=graph)
            med, q1, q3 = timed(lambda: learner.learn(b), args.iters, args.warmup)
            print(json.dumps({'measurement': 'dqn_learn_' + ('graph' if graph else 'eager'),
                              'noisy': noisy_on, 'pixel': bool(args.pixel), 'median_ms': round(med, 4),
                              'q1_ms': round(q1, 4), 'q3_ms': round(q3, 4), 'iters': args.iters}),
                  flush=True)
            del learner


def noisy_bf16_layers(args):
    """--noisy --noisy-bf16[-all]: smi_noisy_forward and smi_noisy_backward_input against their
    _bf16 twins, alternating, at the FC shapes of the DQN models (512 rows, and the 32768 sample
    rows of implicit heads at B = 512, N = 64)"""
    p, st = L.ptr, L.stream()
    L.ensure_workspace('cuda')                # the split reductions need it
    g = torch.Generator().manual_seed(0)
    for R, K, N in ((512, 17, 256), (512, 128, 128), (512, 128, 6), (512, 512, 6), (512, 3136, 1024),
                    (32768, 128, 128), (32768, 128, 6)):
        x, y = torch.randn(R, K, generator=g).cuda(), torch.zeros(R, N).cuda()
        w, ws, b, bs = (torch.randn(*sh, generator=g).cuda() / K ** 0.5 for sh in ((N, K), (N, K), (N,), (N,)))
        fi, fo = torch.randn(K, generator=g).cuda(), torch.randn(N, generator=g).cuda()
        dy, dx = torch.randn(R, N, generator=g).cuda(), torch.zeros(R, K).cuda()

        def fwd(sfx):
            def run():
                for _ in range(args.calls):
                    L.call('smi_noisy_forward' + sfx, p(x), K, R, K, p(w), p(ws), K, p(b), p(bs), p(fi),
                           p(fo), N, 1, p(y), N, st)
            return run

        def bwd(sfx):
            def run():
                for _ in range(args.calls):
                    L.call('smi_noisy_backward_input' + sfx, p(dy), N, R, N, p(w), p(ws), K, K, p(fi),
                           p(fo), p(x), K, p(dx), K, st)
            return run
        for name, mk in (('noisy_forward', fwd), ('noisy_backward_input', bwd)):
            res = timed_alternating([mk(''), mk('_bf16')], args.iters, args.warmup)
            for arm, t in zip(('fp32', 'bf16'), res):
                med, q1, q3 = (1e3 * v / args.calls for v in t)
                print(json.dumps({'measurement': name, 'noisy_dtype': arm, 'rows': R, 'in': K, 'out': N,
                                  'median_us_per_call': round(med, 2), 'q1_us': round(q1, 2),
                                  'q3_us': round(q3, 2), 'calls_per_sample': args.calls,
                                  'iters': args.iters}), flush=True)


def fc_main(args):
    """--fc-bf16: the FC layers and learn() with model.fc_dtype 'fp32' and 'bf16', alternating"""
    p, st = L.ptr, L.stream()
    g = torch.Generator().manual_seed(0)
    for R, K, N in ((512, 17, 256), (512, 128, 128), (512, 128, 6), (512, 512, 6), (512, 3136, 1024),
                    (32768, 128, 128), (32768, 128, 6)):
        x, y = torch.randn(R, K, generator=g).cuda(), torch.zeros(R, N).cuda()
        w, b = (torch.randn(*sh, generator=g).cuda() / K ** 0.5 for sh in ((N, K), (N,)))
        dy, dx = torch.randn(R, N, generator=g).cuda(), torch.zeros(R, K).cuda()

        def fwd(sfx):
            def run():
                for _ in range(args.calls):
                    L.call('smi_linear_forward' + sfx, p(x), K, R, K, p(w), K, p(b), N, 1, p(y), N, st)
            return run

        def bwd(sfx):
            def run():
                for _ in range(args.calls):
                    L.call('smi_linear_backward_input' + sfx, p(dy), N, R, N, p(w), K, K, p(x), K, p(dx),
                           K, st)
            return run
        for name, mk in (('linear_forward', fwd), ('linear_backward_input', bwd)):
            res = timed_alternating([mk(''), mk('_bf16')], args.iters, args.warmup)
            for dtype, t in zip(('fp32', 'bf16'), res):
                med, q1, q3 = (1e3 * v / args.calls for v in t)
                print(json.dumps({'measurement': name, 'fc_dtype': dtype, 'rows': R, 'in': K, 'out': N,
                                  'median_us_per_call': round(med, 2), 'q1_us': round(q1, 2),
                                  'q3_us': round(q3, 2), 'calls_per_sample': args.calls,
                                  'iters': args.iters}), flush=True)
    fc_learn(args, ('fp32', 'bf16'))


def fc_all_main(args):
    """--fc-bf16-all: smi_linear_backward_weight against its _bf16 twin, alternating (single calls
    per layer; the three small 512-row layers also as one grouped fp32 launch against three bf16
    calls), then learn() with model.fc_dtype 'bf16' and 'bf16_all'"""
    p, st = L.ptr, L.stream()
    L.ensure_workspace('cuda')                # the learners' workspace: the row slabs need it
    g = torch.Generator().manual_seed(0)

    def dw_call(sfx, t):
        dy, x, dw, db = t
        (R, N), K = dy.shape, x.shape[1]
        L.call('smi_linear_backward_weight' + sfx, p(dy), N, R, N, p(x), K, K, p(dw), K, p(db), 0, st)

    def report(name, res, **kw):
        for dtype, t in zip(('fp32', 'bf16'), res):
            med, q1, q3 = (1e3 * v / args.calls for v in t)
            print(json.dumps(dict({'measurement': name, 'fc_dtype': dtype}, **kw,
                                  median_us_per_call=round(med, 2), q1_us=round(q1, 2),
                                  q3_us=round(q3, 2), calls_per_sample=args.calls, iters=args.iters)),
                  flush=True)
    small = []
    for R, K, N in ((512, 17, 256), (512, 128, 128), (512, 512, 6), (512, 3136, 1024),
                    (32768, 128, 128), (32768, 128, 6)):
        t = (torch.randn(R, N, generator=g).cuda(), torch.randn(R, K, generator=g).cuda(),
             torch.zeros(N, K).cuda(), torch.zeros(N).cuda())
        if R == 512 and K * N < 1 << 20:
            small.append(t)

        def one(sfx, t=t):
            def run():
                for _ in range(args.calls):
                    dw_call(sfx, t)
            return run
        report('linear_backward_weight', timed_alternating([one(''), one('_bf16')], args.iters, args.warmup),
               rows=R, out=N, **{'in': K})

    def grouped():
        for _ in range(args.calls):
            with L.dw_group(st):
                for t in small:
                    dw_call('', t)

    def apart():
        for _ in range(args.calls):
            for t in small:
                dw_call('_bf16', t)
    report('linear_backward_weight_small3', timed_alternating([grouped, apart], args.iters, args.warmup),
           rows=512, layers='17->256, 128->128, 512->6: fp32 one grouped launch, bf16 three calls')
    fc_learn(args, ('bf16', 'bf16_all'))


def fc_learn(args, arms):
    """learn() with model.fc_dtype on the two arms, alternating step by step"""
    D, A, shape = 17, 6, (4, 84, 84)
    cases = []
    for B in (32, 512):
        lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
        lc.replay.batch_size = B
        lc.model.convs, lc.model.fc_hidden_sizes, lc.model.conv_dtype = NATURE, [512], 'bf16'
        cases.append(('dqn_pixel_learn', B, lc, discrete_pixel_env_config(shape, A),
                      pixel_batch(B, shape, A, 0)))
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = 512
    lc.model.fc_hidden_sizes = [128, 128]
    lc.algo.distributional.update(enabled=True, kind='implicit', atoms=64)
    cases.append(('dqn_implicit64_learn', 512, lc, discrete_env_config(D, A), dqn_batch(512, D, A, 0)))
    for name, B, lc, ec, b in cases:
        for graph in (False, True):
            learners = []
            for dtype in arms:
                lc.model.fc_dtype = dtype
                learners.append(DQNLearner(lc, ec, seed=0, use_graph=graph))
            res = timed_alternating([lambda ln=ln: ln.learn(b) for ln in learners], args.iters,
                                    args.warmup)
            for dtype, (med, q1, q3) in zip(arms, res):
                print(json.dumps({'measurement': name +('_graph' if graph else '_eager'), 'B': B,
                                  'fc_dtype': dtype, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                                  'q3_ms': round(q3, 4), 'iters': args.iters}), flush=True)
            del learners


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--pixel', action='store_true')
    ap.add_argument('--conv-bf16', action='store_true',
                    help='--pixel with model.conv_dtype = bf16 next to the fp32 step')
    ap.add_argument('--gpus', type=int, default=1,
                    help='N >= 2: the data-parallel loop, one process per GPU')
    ap.add_argument('--atoms', type=int, default=0,
                    help='N: the categorical (C51) head with N atoms instead of scalar heads')
    ap.add_argument('--quantiles', type=int, default=0,
                    help='N: the quantile (QR-DQN) head with N quantiles instead of scalar heads')
    ap.add_argument('--implicit', action='store_true',
                    help='the implicit quantile (IQN) head; --atoms N is its sample count (8)')
    ap.add_argument('--noisy', action='store_true',
                    help='noisy linear layers against the plain ones; combines with --atoms, '
                         '--quantiles, --implicit and --pixel')
    ap.add_argument('--noisy-bf16', action='store_true',
                    help="--noisy with model.noisy.dtype = 'bf16' against 'fp32': the noisy layers and learn()")
    ap.add_argument('--noisy-bf16-all', action='store_true',
                    help="--noisy with model.noisy.dtype = 'bf16_all' against 'fp32'")
    ap.add_argument('--fc-bf16', action='store_true',
                    help="model.fc_dtype = 'bf16' against 'fp32': the FC layers and learn()")
    ap.add_argument('--fc-bf16-all', action='store_true',
                    help="model.fc_dtype = 'bf16_all' against 'bf16': the FC weight gradients and learn()")
    ap.add_argument('--kappa', type=float, default=1.0,
                    help='--quantiles: the Huber threshold (0: the pinball loss)')
    ap.add_argument('--calls', type=int, default=20,
                    help='--atoms / --quantiles: back-to-back kernel calls per timed sample')
    args = ap.parse_args()
    if args.gpus != 1:
        return dp_main(args)
    if args.fc_bf16_all:
        return fc_all_main(args)
    if args.fc_bf16:
        return fc_main(args)
    if args.noisy or args.noisy_bf16 or args.noisy_bf16_all:
        return noisy_main(args)
    if args.implicit:
        return implicit_main(args)
    if args.atoms or args.quantiles:
        return dist_main(args)
    if args.pixel or args.conv_bf16:
        return pixel_main(args)
    B, D, A = 512, 17, 6
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    lc.model.fc_hidden_sizes = [128, 128]
    b = dqn_batch(B, D, A, 0)
    for name, graph in (('dqn_learn_eager', False), ('dqn_learn_graph', True)):
        learner = DQNLearner(lc, discrete_env_config(D, A), seed=0, use_graph=graph)
        extra = {}
        if not graph:
            learner.learn(b)
            extra['launches_per_step'], extra['library_calls_per_step'] = \
                count_launches(lambda: learner.learn(b))
        med, q1, q3 = timed(lambda: learner.learn(b), args.iters, args.warmup)
        print(json.dumps(dict({'measurement': name, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                               'q3_ms': round(q3, 4), 'iters': args.iters}, **extra)), flush=True)
    dlc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
    dlc.replay.batch_size = B
    db = {k: v.cuda() for k, v in synthetic.ddpg_batch(B, D, A, seed=0).items()}
    for name, graph in (('ddpg_c4_learn_eager', False), ('ddpg_c4_learn_graph', True)):
        learner = DDPGLearner(dlc, gym_env_config(D, A), seed=0, use_graph=graph)
        med, q1, q3 = timed(lambda: learner.learn(db), args.iters, args.warmup)
        print(json.dumps({'measurement': name, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                          'q3_ms': round(q3, 4), 'iters': args.iters}), flush=True)


if __name__ == '__main__':
    main()
