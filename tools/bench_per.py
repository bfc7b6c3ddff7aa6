"""Per-launch times of the prioritized replay kernels at the reference size.

Shape: capacity 2^19, len 333,333 (the reference memory_size), batch 512, leaves
from a spread of priorities (1e-3 .. 1e1, ** alpha 0.6).  Each figure is the
median of --iters repeats (default 40) of ONE launch between two HIP events,
after warm-up, with min / max and quartiles:

  per_sample      smi_per_sample, batch 512, beta 0.4
  per_update_td   smi_per_update_td, 512 TD errors at freshly drawn indices
  per_insert      smi_per_insert of 512 rows
  mt_randint      smi_mt_randint at the same batch: the uniform draw it stands in for
  learn_c4        DDPGLearner.learn() of the C4 workload (batch 512, obs 17, act 6),
                  events around the whole call, same process
  per_ref_host    tests/per_ref.py, one batch on the host (context; wall clock)

and the sample + update overhead as a fraction of learn_c4.  One JSON line per
figure on stdout and, with --out, appended to that file.
"""
import argparse
import copy
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from surreal_amd import _lib as L  # noqa: E402


def timed(fn, iters, warm=5):
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
    return sorted(s.elapsed_time(e) * 1e3 for s, e in evs)          # us


def summary(us):
    q = lambda f: us[min(len(us) - 1, int(f * len(us)))]  # noqa: E731
    return {'median_us': round(us[len(us) // 2], 2), 'min_us': round(us[0], 2),
            'max_us': round(us[-1], 2), 'q1_us': round(q(0.25), 2), 'q3_us': round(q(0.75), 2),
            'repeats': len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--cap-log2', type=int, default=19)
    ap.add_argument('--len', type=int, default=333333)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    L.require_gpu()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    L.ensure_workspace(dev)
    st, P = L.stream(dev), L.ptr
    cap, n, B, alpha = 1 << args.cap_log2, args.len, args.batch, 0.6
    lines = []

    def emit(name, us=None, **extra):
        out = {'kernel': name, 'capacity': cap, 'len': n, 'batch': B}
        if args.tag:
            out['tag'] = args.tag
        if us is not None:
            out.update(summary(us))
        out.update(extra)
        lines.append(out)
        print(json.dumps(out), flush=True)

    tree = torch.empty(int(L.lib().smi_per_tree_doubles(cap)), dtype=torch.float64, device=dev)
    L.call('smi_per_init', P(tree), cap, st)
    prio = 10.0 ** np.random.RandomState(0).uniform(-3.0, 1.0, size=n)
    leaves = torch.as_tensor(prio ** alpha, device=dev)
    slots = torch.arange(n, dtype=torch.int64, device=dev)
    L.call('smi_per_set', P(tree), cap, P(slots), P(leaves), n, st)
    host = np.zeros(625, dtype=np.uint32)
    L.check(L.lib().smi_mt_seed(0, host.ctypes.data), 'smi_mt_seed')
    state = torch.from_numpy(host.view(np.int32).copy()).to(dev)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    w = torch.empty(B, dtype=torch.float32, device=dev)
    td = torch.randn(B, device=dev)

    sample = lambda: L.call('smi_per_sample', P(tree), cap, n, P(state), B, 0.4, P(idx), P(w), st)  # noqa
    us_s = timed(sample, args.iters)
    emit('per_sample', us_s, beta=0.4)
    update = lambda: L.call('smi_per_update_td', P(tree), cap, P(idx), P(td), 1, B, 1e-6, alpha, st)  # noqa
    us_u = timed(update, args.iters)
    emit('per_update_td', us_u, alpha=alpha)
    pos = [0]

    def insert():
        L.call('smi_per_insert', P(tree), cap, pos[0], B, n, alpha, st)
        pos[0] = (pos[0] + B) % n
    emit('per_insert', timed(insert, args.iters), rows=B, alpha=alpha)
    uni = lambda: L.call('smi_mt_randint', P(state), n, B, P(idx), st)  # noqa
    emit('mt_randint', timed(uni, args.iters))

    from surreal_amd import synthetic
    from surreal_amd.config import DDPG_DEFAULT_LEARNER_CONFIG, gym_env_config
    from surreal_amd.ddpg import DDPGLearner
    lc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    learner = DDPGLearner(lc, gym_env_config(17, 6), seed=1, device=dev)
    batch = {k: v.to(dev) for k, v in synthetic.ddpg_batch(B, 17, 6, seed=0).items()}
    batch['weights'] = torch.rand(B, 1, device=dev) + 0.05
    us_l = timed(lambda: learner.learn(batch), args.iters)
    emit('learn_c4', us_l, weighted=True)
    frac = (us_s[len(us_s) // 2] + us_u[len(us_u) // 2]) / us_l[len(us_l) // 2]
    emit('overhead', sample_plus_update_over_learn=round(frac, 4))

    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import per_ref
    t = tree.cpu().numpy()
    ref = per_ref.PerRef.from_leaves(cap, t[2 * cap::2], max_priority=float(t[0]))
    random.seed(0)
    t0 = time.perf_counter()
    got, _ = ref.sample(n, B, 0.4)
    ref.update_from_td(got, td.cpu().numpy(), 1e-6, alpha)
    emit('per_ref_host', wall_us=round((time.perf_counter() - t0) * 1e6, 1),
         note='one sample + update of the batch in Python on the host (wall clock, one run)')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for o in lines:
                f.write(json.dumps(o) + '\n')


if __name__ == '__main__':
    main()
