"""Data-parallel DDPGLearner with a prioritized replay: ranks are simulated in
one process by driving each learner's _learn_phases in lockstep and summing the
yielded exchange images, as the all-reduce does (tests/dp_harness.py
lockstep).  N ranks on 96 / N rows each must end bit-identical, hold the TD
errors of the whole draw in draw order, and land where one learner on the 96
rows lands: rank 0 goes through the bar of tests/test_gpu_per.py::
test_random_weights_on_the_envelope against the fp64 weighted oracle on the
GLOBAL batch.  Replicated priority trees fed from td_error stay bit-identical."""
import random

import numpy as np
import pytest
import torch

from surreal_amd import synthetic
from surreal_amd.config import gym_env_config
from surreal_amd.ddpg import DDPGLearner
from surreal_amd.replay import PrioritizedReplay
from tests import parity as P
from tests import per_ref as PR
from tests import test_gpu_ddpg as T
from tests.dp_harness import Group as _Group, cut as _cut, lockstep as _lockstep, pad4
from tests.dp_harness import to_dev as _dev
from tests.helpers import per_cfg as _per_cfg, replay_rows as _rows
from tests.test_gpu_per import WeightedRef

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BG, D, A = 96, 17, 6


class _Seeded(object):
    """a rank as _lockstep sees it, with numpy's global stream seeded as the
    rank's own process would have it when its launches begin (the TD3 smoothing
    noise is a host draw of the global batch's rows on every rank)"""

    def __init__(self, learner, seed):
        self.learner, self.seed = learner, seed

    def _learn_phases(self, batch):
        np.random.seed(self.seed)
        yield from self.learner._learn_phases(batch)


def _ranks(lc_of, ec, world, seed=2):
    return [DDPGLearner(lc_of(BG // world), ec, seed=seed, dp=_Group(world, r)) for r in range(world)]


def _step(learners, shards, seed):
    return _lockstep([_Seeded(l, seed) for l in learners], shards)


def _state(learner):
    out = dict(T._ddpg_state(learner))
    for name, o in learner.opt.items():
        for k in ('m', 'v', 'step'):
            out[f'{name}.{k}'] = o[k].detach().cpu().clone()
    out['stats_buf'] = learner.stats_buf.detach().cpu().clone()
    out['td_error'] = learner.td_error.detach().cpu().clone()
    return out


def _assert_same(a, b, tag):
    sa, sb = _state(a), _state(b)
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (tag, k)


def _batch(it, B=BG):
    return {k: v.numpy() for k, v in synthetic.ddpg_batch(B, D, A, seed=it).items()}


# --------------------------------------------------------------- envelope
@pytest.mark.parametrize('world', [2, 3, 4])
@pytest.mark.parametrize('td3', [False, True], ids=['plain', 'td3'])
def test_dp_random_weights_on_the_envelope(td3, world):
    iters, n = 2, BG // world
    lc_of = lambda B: _per_cfg(B, double=td3, action_reg=td3)  # noqa: E731
    lc = lc_of(BG)
    learners = _ranks(lc_of, gym_env_config(D, A), world)
    l0 = learners[0]
    init = {k: v for k, v in T._ddpg_state(l0).items() if k in ('actor', 'critic', 'critic2')}
    batches = [_batch(it) for it in range(iters)]
    ws = [np.random.RandomState(70 + it).uniform(0.05, 1.0, size=BG).astype(np.float32)
          for it in range(iters)]
    r64 = WeightedRef(lc, D, A, dtype=torch.float64)
    T._load_ddpg(r64, init)
    vs = [T._DVariant('order', k, lc, D, A, init) for k in T.DDPG_ORDERS]
    vs += [T._DVariant('ulp', k, lc, D, A, init) for k in range(1, 7)]
    for v in vs:
        v.ref.__class__ = WeightedRef
        v.ref.weight_noise = v._noisy if v.kind == 'ulp' else None
    # the exchange image: [critic | critic2 | pad to 4 floats | td_all]
    ng = l0.model.critic.flat.numel() * (2 if td3 else 1)
    ng4 = pad4(ng)
    report = {}
    for it, b in enumerate(batches):
        dev = _dev(b)
        dev['weights'] = torch.as_tensor(ws[it]).to(DEV).view(BG, 1)
        assert _step(learners, [_cut(dev, r, n) for r in range(world)], 100 + it) == 2
        for r, l in enumerate(learners):
            _assert_same(l, l0, (it, r))
            assert tuple(l.td_error.shape) == (BG,)
            own = (l._bufs['c_q'] - l._bufs['y']).view(-1)
            assert tuple(own.shape) == (n,)
            assert torch.equal(l.td_error[r * n:(r + 1) * n].view(torch.int32), own.view(torch.int32))
            base = l._critic_pack.data_ptr()
            assert l._critic_pack.numel() == ng4 + BG
            assert l.opt['critic']['g'].data_ptr() == base
            assert l.td_error.data_ptr() == base + 4 * ng4
        got, got_grad = T._ddpg_state(l0), l0.opt['critic']['g'].detach().cpu().numpy()
        np.random.seed(100 + it)
        f64 = lambda k: torch.as_tensor(b[k], dtype=torch.float32).double()  # noqa: E731
        r64.weights = ws[it]
        r64.optimize(f64('obs'), f64('actions'), f64('rewards'), f64('obs_next'), f64('dones'))
        for v in vs:
            np.random.seed(100 + it)
            v.ref.weights = ws[it]
            v.optimize(b, it)
        if it == 0:
            wd, sc = P.width(r64.critic_grad, [v.ref.critic_grad for v in vs])
            P.check('critic_grad@0', got_grad, r64.critic_grad, wd, sc, report)
        p64 = T._ddpg_ref_state(r64)
        pvs = [T._ddpg_ref_state(v.ref) for v in vs]
        for k in p64:
            wd, sc = P.width(p64[k], [x[k] for x in pvs])
            P.check(f'{k}@{it}', got[k], p64[k], wd, sc, report)
    P.print_report(report)


def test_dp_unit_weights_change_nothing():
    world, n = 2, BG // 2
    lc_of = lambda B: _per_cfg(B, double=True)  # noqa: E731
    plain = _ranks(lc_of, gym_env_config(D, A), world, seed=3)
    unit = _ranks(lc_of, gym_env_config(D, A), world, seed=3)
    ones = torch.ones(BG, 1, device=DEV)
    for it in range(2):
        dev = _dev(_batch(10 + it))
        assert _step(plain, [_cut(dev, r, n) for r in range(world)], it) == 2
        assert _step(unit, [_cut(dict(dev, weights=ones), r, n) for r in range(world)], it) == 2
        for a, b in zip(plain, unit):
            _assert_same(a, b, it)


# ---------------------------------------------------------------- PER loop
def _per_step(reps, learners, Bg, beta, seed, want=None):
    """sample_shard -> learn -> update_priorities_from_td on every replica"""
    world = len(reps)
    shards, idxs = [], []
    for r, rep in enumerate(reps):
        idx_all, batch = rep.sample_shard(Bg, r, world, beta=beta)
        if want is not None:
            assert idx_all.cpu().tolist() == want, r
        assert tuple(batch['weights'].shape) == (Bg // world, 1)
        shards.append(batch)
        idxs.append(idx_all)
    assert _step(learners, shards, seed) == 2
    for rep, idx_all, l in zip(reps, idxs, learners):
        rep.update_priorities_from_td(idx_all, l.td_error, eps=1e-6)
    for rep in reps[1:]:
        assert torch.equal(rep.tree.view(torch.int64), reps[0].tree.view(torch.int64))
        assert torch.equal(rep.rng.dev, reps[0].rng.dev)
        assert rep.max_priority == reps[0].max_priority


def test_dp_prioritized_replay_loop():
    """two replicas (same seed, same inserts), world 2.  Each draw is
    tests/per_ref.py's from the device's own leaves; the trees, generators and
    max_priority stay bit-identical; the drawn leaves are (|td| + 1e-6) ** 0.6
    within the 2^-51 rule of test_gpu_dqn.py::test_prioritized_replay_loop."""
    world, n, seed = 2, 150, 4321
    lc_of = lambda B: _per_cfg(B, 200)  # noqa: E731
    ec = gym_env_config(D, A)
    reps = [PrioritizedReplay(lc_of(BG // world), ec, seed=seed) for _ in range(world)]
    rows = _rows(n, D, A, 3)
    for rep in reps:
        rep.insert_rows(rows)
    learners = _ranks(lc_of, ec, world, seed=1)
    cap = reps[0].capacity
    random.seed(seed)
    for it in range(3):
        want, _ = PR.ref_from_device(reps[0].tree, cap)[0].sample(n, BG, 0.4)
        _per_step(reps, learners, BG, 0.4, it, want)
        _assert_same(learners[0], learners[1], it)
        PR.check_drawn_leaves(reps[0].tree, cap, want, learners[0].td_error.cpu().numpy())


def test_dp_pixel_frame_shared_loop():
    """frame-shared PrioritizedReplay replicas feeding pixel learners (9 x 20 x
    20 camera, 3 stacked frames), world 2: ranks bit-identical, perception and
    its target included, and so are the trees"""
    from tests.test_gpu_replay_shared import _cfg, _env, _exps, rolling_stream
    world, Bg, Dp, Ap, cam, mem = 2, 16, 5, 2, (9, 20, 20), 40
    ec = _env(Dp, Ap, cam)
    lc = _cfg(Bg // world, mem, share=True, frame_slots=4 * mem)
    exps, _ = _exps(rolling_stream(1, 30, (3, 20, 20), seed=8), Dp, Ap, seed=9)
    reps = [PrioritizedReplay(lc, ec, seed=5) for _ in range(world)]
    for rep in reps:
        rep.insert_rows(*rep.pack(exps))
        assert rep.share_frames
    learners = [DDPGLearner(lc, ec, seed=0, dp=_Group(world, r)) for r in range(world)]
    assert learners[0].is_pixel_input
    start = _state(learners[0])
    for it in range(2):
        _per_step(reps, learners, Bg, 0.4, it)
        _assert_same(learners[0], learners[1], it)
        assert tuple(learners[0].td_error.shape) == (Bg,)
    end = _state(learners[0])
    assert {'perc', 'perc_t'} <= set(end)
    assert not torch.equal(end['perc'], start['perc'])               # and the perception trained
    assert torch.equal(end['perc'], end['perc_t'])                   # hard update at step 2


# ---------------------------------------------------------- unchanged paths
def test_without_dp_nothing_is_exchanged_and_dp_checks_the_row_count():
    B = 64
    lc, ec = _per_cfg(B), gym_env_config(D, A)
    phased, plain = DDPGLearner(lc, ec, seed=3), DDPGLearner(lc, ec, seed=3)
    one = DDPGLearner(lc, ec, seed=3, dp=_Group(1, 0))
    assert phased.dp is None and one.dp is None
    for it in range(2):
        dev = _dev(_batch(20 + it, B))
        dev['weights'] = torch.rand(B, 1, generator=torch.Generator().manual_seed(it)).to(DEV) + 0.05
        assert list(phased._learn_phases(dev)) == []
        assert list(one._learn_phases(dev)) == []
        plain.learn(dev)
        assert phased.current_iteration == it + 1
        assert tuple(phased.td_error.shape) == (B,)
        _assert_same(phased, plain, it)
        _assert_same(one, plain, it)
    dp = DDPGLearner(_per_cfg(32), ec, seed=3, dp=_Group(2, 1))
    assert tuple(dp.td_error.shape) == (64,)
    before = _state(dp)
    bad = _dev(_batch(0, 48))
    with pytest.raises(ValueError, match='batch_size'):
        list(dp._learn_phases(bad))
    with pytest.raises(ValueError, match='batch_size'):
        dp.learn(bad)
    torch.cuda.synchronize()
    after = _state(dp)
    assert all(torch.equal(before[k], after[k]) for k in before)       # nothing was launched
