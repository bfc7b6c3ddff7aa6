"""What the data-parallel tests share: ranks simulated in one process (a fake
group, _learn_phases driven in lockstep with the yielded buffers summed as the
all-reduce sums them), ranks as real processes over torch.distributed
(spawn_ranks), and the batch cutting both need."""
import os
import socket
import tempfile

import torch
import torch.multiprocessing as mp


class Group(object):
    """a data-parallel group whose ranks are driven through _learn_phases"""

    def __init__(self, world, rank=0):
        self.world_size, self.rank = world, rank

    def allreduce_(self, t):
        raise AssertionError('ranks are driven through _learn_phases in this test')


def lockstep(learners, shards):
    """one learn() of every rank, the exchanges summed; returns their number"""
    gens = [l._learn_phases(s) for l, s in zip(learners, shards)]
    nphase = 0
    while True:
        bufs, done = [], 0
        for g in gens:
            try:
                bufs.append(next(g))
            except StopIteration:
                done += 1
        if done:
            assert done == len(gens)
            return nphase
        total = bufs[0].clone()
        for b in bufs[1:]:
            total += b
        for b in bufs:
            b.copy_(total)
        nphase += 1


def cut(x, r, n):
    """rows [r * n, (r + 1) * n) of every tensor of a batch (dicts and lists nest)"""
    if x is None:
        return None
    if isinstance(x, dict):
        return {k: cut(v, r, n) for k, v in x.items()}
    if isinstance(x, list):
        return [cut(v, r, n) for v in x]
    return x[r * n:(r + 1) * n].contiguous()


def to_dev(b, device='cuda'):
    """a host batch on the device: uint8 stays uint8, the rest becomes float32"""
    return {k: torch.as_tensor(v).to(device) if torch.as_tensor(v).dtype == torch.uint8
            else torch.as_tensor(v, dtype=torch.float32).to(device) for k, v in b.items()}


def pad4(n):
    """where the tails of an exchange image start: n floats up to a multiple of 4"""
    return (n + 3) // 4 * 4


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, backend, outdir, worker, args):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    torch.save(worker(rank, world, *args), os.path.join(outdir, f'rank{rank}.pt'))
    dist.destroy_process_group()


def spawn_ranks(worker, world, *args, backend='gloo'):
    """worker(rank, world, *args) in `world` processes that share cuda:0, inside
    an initialised process group; returns what each rank returned (it travels
    through torch.save / torch.load(weights_only=True)), in rank order"""
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_rank_main, args=(world, free_port(), backend, outdir, worker, args),
                 nprocs=world, join=True)
        return [torch.load(os.path.join(outdir, f'rank{r}.pt'), weights_only=True)
                for r in range(world)]
