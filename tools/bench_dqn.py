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

--gpus N (2 <= N <= 16) times the data-parallel loop instead: one process per
GPU (torch.multiprocessing spawn, 'nccl' = RCCL), each with one
DQNLearner(dp=TorchDistAllReduce()) and one PrioritizedReplay replica, a step
being sample_shard -> learn -> update_priorities_from_td at a global batch of
512 (512 / N rows per rank).  Rank 0 prints the one JSON line.  With fewer than
N (or fewer than two) GPUs visible it says so and starts nothing.

Usage: python tools/bench_dqn.py [--iters 40] [--warmup 10] [--pixel | --gpus N]
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
        for name, graph in (('dqn_pixel_learn_eager', False), ('dqn_pixel_learn_graph', True)):
            learner = DQNLearner(lc, ec, seed=0, use_graph=graph)
            extra = {}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--pixel', action='store_true')
    ap.add_argument('--gpus', type=int, default=1,
                    help='N >= 2: the data-parallel loop, one process per GPU')
    args = ap.parse_args()
    if args.gpus != 1:
        return dp_main(args)
    if args.pixel:
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
