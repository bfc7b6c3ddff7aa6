#!/usr/bin/env python3
"""Dumps what two learn() calls of the LSTM learner leave, for a list of small
configurations that between them reach both sides of every host-side rule of
csrc/ppo_rnn.hip (fused clip norm, GAE + PREP in one recurrence, the policy
gradient as the head chain's prologue, the fused decision, the value
statistics' source), so two checkouts can be compared byte for byte:

    python tools/rnn_ab_dump.py OUTDIR          # in each checkout
    python tools/rnn_ab_dump.py --compare A B   # every array of A against B

Only the public Python API is used (PPOLearner, synthetic batches), so the
script runs unchanged against an older checkout: run it with that checkout's
root as the working directory.  Per configuration it writes
OUTDIR/<name>/<array>.npy: every published module's state_dict, both
optimizers' moments and step counters, and last_stats() after each call.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())

CAM = (3, 84, 84)
BASE = dict(mode='adapt', B=19, T=8, horizon=3, D=11, A=4, Hd=24, hidden=(32, 32), layers=1, F=0,
            rnn=True, world=1, prep_side=False, epochs=(3, 3))
# name -> overrides of BASE (tests/test_gpu_rnn.py::test_rnn_learn_small_matches_oracle's shape)
CONFIGS = {
    'clip_a4': dict(mode='clip'),
    'adapt_a4': dict(),
    'adapt_a8_d12': dict(A=8, D=12),               # the policy prologue rides the fused head chain
    'adapt_heads_520_32': dict(hidden=(520, 32)),  # a head outside the dW group: no fused clip norm
    'adapt_heads_30_18': dict(hidden=(30, 18)),    # the layer-GEMM head path
    'clip_heads_30_18': dict(mode='clip', hidden=(30, 18)),
    'adapt_two_layers': dict(layers=2),
    'clip_two_layers': dict(mode='clip', layers=2),
    # tests/test_gpu_cnn.py's smallest learns: the pixel stem under the LSTM, and under the MLP policy
    'adapt_pixel': dict(B=6, T=6, horizon=2, D=7, A=3, Hd=16, hidden=(16, 16), F=32, epochs=(2, 2)),
    'clip_pixel_mlp': dict(mode='clip', B=24, T=6, horizon=6, D=7, A=3, Hd=0, hidden=(32, 24), F=32,
                           rnn=False, epochs=(1, 1)),
    'adapt_prep_side': dict(prep_side=True),       # PREP on its own stream: no dual recurrence
    # two ranks holding the same shard (the all-reduce doubles): the exchange side of every rule
    'adapt_two_ranks': dict(world=2),
    'clip_two_ranks': dict(world=2, mode='clip'),
}


class MirrorGroup(object):
    """A data-parallel group of `n` ranks that all hold this rank's shard."""

    def __init__(self, n):
        self.world_size = n

    def allreduce_(self, t):
        return t.mul_(self.world_size)


def run(name, outdir):
    import torch
    from surreal_amd import synthetic
    from surreal_amd.config import PPO_DEFAULT_LEARNER_CONFIG, gym_env_config, pixel_env_config
    from surreal_amd.learner import PPOLearner
    import copy
    c = dict(BASE, **CONFIGS[name])
    lc = copy.deepcopy(PPO_DEFAULT_LEARNER_CONFIG)
    lc.model.actor_fc_hidden_sizes = list(c['hidden'])
    lc.model.critic_fc_hidden_sizes = list(c['hidden'])
    lc.model.cnn_feature_dim = c['F'] or 256
    lc.algo.use_z_filter = True
    lc.algo.n_step = c['T']
    lc.algo.ppo_mode = c['mode']
    lc.algo.advantage.lam = 1.0 if c['rnn'] else 0.95
    lc.algo.rnn.if_rnn_policy = bool(c['rnn'])
    lc.algo.rnn.rnn_hidden = c['Hd']
    lc.algo.rnn.rnn_layer = c['layers']
    lc.algo.rnn.horizon = c['horizon']
    lc.algo.consts.epoch_policy, lc.algo.consts.epoch_baseline = c['epochs']
    lc.replay.batch_size = c['B']
    pixel = CAM if c['F'] else None
    ec = pixel_env_config(c['D'], c['A'], CAM) if pixel else gym_env_config(c['D'], c['A'])
    os.environ['SMI_PREP_SIDE'] = '1' if c['prep_side'] else '0'   # read by the constructor
    dp = MirrorGroup(c['world']) if c['world'] > 1 else None
    learner = PPOLearner(lc, ec, seed=5, dp=dp)
    arrays = {}
    for it in range(2):
        kw = dict(pixel=pixel) if pixel else {}
        batch = synthetic.ppo_batch(c['B'], c['T'], c['D'], c['A'], seed=100 + it,
                                    rnn_hidden=c['Hd'] if c['rnn'] else None,
                                    rnn_layers=c['layers'], **kw)
        learner.learn(synthetic.to_device(batch, 'cuda'))
        stats = learner.last_stats()
        keys = sorted(stats)
        arrays[f'stats_{it}'] = np.asarray([float(stats[k]) for k in keys], dtype=np.float64)
        arrays[f'stats_raw_{it}'] = learner.stats_buf.detach().cpu().numpy().copy()
    for mname, mod in learner.module_dict().items():
        for key, t in mod.state_dict().items():
            arrays[f'{mname}.{key}'] = t.detach().cpu().numpy()
    # optimizer state: every tensor attribute of the learner whose name says so
    for attr, v in sorted(vars(learner).items()):
        if torch.is_tensor(v) and any(s in attr for s in ('_m', '_v', 'step', 'adam', 'opt')):
            arrays[f'learner.{attr}'] = v.detach().cpu().numpy()
    d = os.path.join(outdir, name)
    os.makedirs(d, exist_ok=True)
    for n, a in arrays.items():
        np.save(os.path.join(d, n + '.npy'), np.ascontiguousarray(a))
    print(f'{name}: {len(arrays)} arrays, epochs_run {stats.get("epochs_run")}', flush=True)


def compare(a, b):
    bad = total = 0
    for name in sorted(os.listdir(a)):
        fa, fb = sorted(os.listdir(os.path.join(a, name))), sorted(os.listdir(os.path.join(b, name)))
        if fa != fb:
            print(f'{name}: different arrays: {sorted(set(fa) ^ set(fb))}')
            bad += 1
        for f in fa:
            if f not in fb:
                continue
            with open(os.path.join(a, name, f), 'rb') as x, open(os.path.join(b, name, f), 'rb') as y:
                xa, ya = x.read(), y.read()
            total += 1
            same = xa == ya
            bad += not same
            print(f'{name}/{f}: {len(xa)} bytes, {"identical" if same else "DIFFERENT"}')
    print(f'{total} arrays compared, {bad} different')
    return 1 if bad or not total else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for cfg in (sys.argv[2:] or CONFIGS):
        run(cfg, sys.argv[1])
