"""Data-parallel DQNLearner: ranks are simulated in one process by driving each
learner's _learn_phases in lockstep and summing the yielded exchange images, as
the all-reduce does (tests/dp_harness.py lockstep).  N ranks on B / N rows
each must land where one learner on the B rows lands: rank 0 goes through the
single learner's own envelope check on the GLOBAL batches, unchanged, and the
ranks must be bit-identical to each other, priority trees included."""
import copy
import random

import pytest
import torch

from surreal_amd.config import discrete_env_config, discrete_pixel_env_config
from surreal_amd.dqn import DQNLearner
from surreal_amd.replay import PrioritizedReplay, UniformReplay
from tests import dqn_ref as R
from tests import parity as P
from tests import per_ref as PR
from tests import qconv_ref as Q
from tests.dp_harness import Group as _Group, cut as _cut, lockstep as _lockstep, pad4
from tests.dp_harness import to_dev as _dev

pytestmark = pytest.mark.gpu


def _rank_config(lc, world):
    lc = copy.deepcopy(lc)
    lc.replay.batch_size //= world              # each rank's own rows; the target period stays
    return lc


def _load(learner, init):
    learner.q_func.load_state_dict(init['q_func'])
    learner.q_target.load_state_dict(init['q_target'])
    return learner


def _ranks(lc, ec, init, world):
    return [_load(DQNLearner(_rank_config(lc, world), ec, dp=_Group(world, r)), init)
            for r in range(world)]


def _state(learner):
    return {'q_func': R.flat_of(learner.q_func.state_dict()),
            'q_target': R.flat_of(learner.q_target.state_dict())}


def _bits_equal(a, b):
    return all(torch.equal(getattr(a, n).flat, getattr(b, n).flat) for n in ('q_func', 'q_target')) \
        and torch.equal(a.td_error, b.td_error) and torch.equal(a.stats_buf, b.stats_buf)


def _run_lockstep(learners, batches, Bg):
    """3 global batches through the ranks; returns rank 0's envelope triples"""
    world = len(learners)
    n = Bg // world
    got = []
    for it, b in enumerate(batches):
        d = _dev(b)
        assert _lockstep(learners, [_cut(d, r, n) for r in range(world)]) == 1    # ONE exchange
        l0 = learners[0]
        assert tuple(l0.td_error.shape) == (Bg,)
        P4 = pad4(l0.q_func.flat.numel())
        base = l0._xbuf.data_ptr()
        assert l0.opt['g'].data_ptr() == base and l0.td_error.data_ptr() == base + 4 * P4
        assert l0.stats_buf.data_ptr() == base + 4 * (P4 + Bg) and l0._xbuf.numel() == P4 + Bg + 2
        got.append((_state(l0), l0.last_stats(), l0.td_error.cpu().double().numpy()))
        for l in learners:
            assert _bits_equal(l, l0), it
            # the target copy falls after the second step, as for one learner
            assert torch.equal(l.q_func.flat, l.q_target.flat) == (it == 1), it
    for l in learners:
        assert l.target_update_tracker.value == 3 * Bg
    return got


# --------------------------------------------------------------- envelope
@pytest.mark.parametrize('world', [2, 3, 4])
@pytest.mark.parametrize('name', ['b96_duel_dq', 'b96_plain', 'three_hidden'])
def test_dp_learn_envelope(name, world):
    lc, D, A, init, batches = R.envelope_case(name)
    Bg = lc.replay.batch_size
    learners = _ranks(lc, discrete_env_config(D, A), init, world)
    got = _run_lockstep(learners, batches, Bg)
    P.print_report(R.envelope_check(lc, D, A, init, batches, got))


def test_dp_pixel_learn_envelope():
    lc, shape, A, init, batches = Q.pix_case('pix_small')
    Bg = lc.replay.batch_size
    learners = _ranks(lc, discrete_pixel_env_config(shape, A), init, 2)
    got = _run_lockstep(learners, batches, Bg)
    P.print_report(Q.envelope_check_pixels(lc, shape, A, init, batches, got))


# ---------------------------------------------------------------- PER loop
def _lowdim_replicas():
    lc, D, A, init, _ = R.envelope_case('b96_duel_dq')
    lc = copy.deepcopy(lc)
    lc.replay.memory_size, lc.replay.sampling_start_size = 400, 10
    ec, n = discrete_env_config(D, A), 300
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(n, 2 * D + 3, generator=g)
    rows[:, D] = torch.randint(0, A, (n,), generator=g).float()
    rows[:, 2 * D + 2] = (torch.rand(n, generator=g) < 0.1).float()
    reps = [PrioritizedReplay(lc, ec, seed=2468) for _ in range(2)]
    for rep in reps:
        rep.insert_rows(rows)
    return lc, ec, init, reps, n, 64, 2468, None


def _frame_shared_replicas():
    lc, shape, A, init, _ = Q.pix_case('pix_small')
    lc = copy.deepcopy(lc)
    lc.replay.memory_size, lc.replay.sampling_start_size, lc.replay.share_frames = 64, 10, True
    ec, n = discrete_pixel_env_config((1,) + shape[1:], A, frame_stacks=4), 40
    g = torch.Generator().manual_seed(4)
    rows = torch.zeros(n, 3)
    rows[:, 0] = torch.randint(0, A, (n,), generator=g).float()
    rows[:, 1] = 1.5 * torch.randn(n, generator=g)
    rows[:, 2] = (torch.rand(n, generator=g) < 0.2).float()
    film = torch.randint(0, 256, (n + 4,) + shape[1:], generator=g, dtype=torch.uint8)
    pix = torch.stack([film[i:i + 4] for i in range(n)])
    pix_next = torch.stack([film[i + 1:i + 5] for i in range(n)])
    reps = [PrioritizedReplay(lc, ec, seed=77) for _ in range(2)]
    for rep in reps:
        rep.insert_rows(rows, pix, pix_next)
        assert rep.share_frames
    return lc, ec, init, reps, n, lc.replay.batch_size, 77, (pix, pix_next)


@pytest.mark.parametrize('make', [_lowdim_replicas, _frame_shared_replicas],
                         ids=['low_dim', 'frame_shared_pixels'])
def test_dp_prioritized_replay_loop(make):
    """two replicas (same seed, same inserts), world 2: sample_shard -> learn ->
    update_priorities_from_td(idx_all, td_error) on both.  The draw is
    tests/per_ref.py's from the device's own leaves, each rank's batch holds its
    slice of the drawn rows, and the trees stay bit-identical, their drawn
    leaves (|td| + 1e-6) ** 0.6 within the 2^-51 rule of
    test_gpu_dqn.py::test_prioritized_replay_loop."""
    lc, ec, init, reps, n, Bg, seed, frames = make()
    world, h = 2, Bg // 2
    learners = _ranks(lc, ec, init, world)
    cap = reps[0].capacity
    random.seed(seed)
    for it in range(3):
        want, _ = PR.ref_from_device(reps[0].tree, cap)[0].sample(n, Bg, 0.4)
        shards, idxs = [], []
        for r, rep in enumerate(reps):
            idx_all, batch = rep.sample_shard(Bg, r, world, beta=0.4)
            assert idx_all.cpu().tolist() == want, (it, r)
            mine = idx_all[r * h:(r + 1) * h]
            got_rows = torch.cat([batch[k] for k in ('actions', 'rewards', 'dones')], 1)
            D = rep.obs_dim
            table = rep.table[mine]
            assert torch.equal(got_rows, torch.cat([table[:, D:D + 2], table[:, 2 * D + 2:]], 1))
            if frames is None:
                assert torch.equal(batch['obs'], table[:, :D])
                assert torch.equal(batch['obs_next'], table[:, D + 2:2 * D + 2])
            else:
                assert torch.equal(batch['obs']['pixel']['camera0'].cpu(), frames[0][mine.cpu()])
                assert torch.equal(batch['obs_next']['pixel']['camera0'].cpu(), frames[1][mine.cpu()])
            assert tuple(batch['weights'].shape) == (h, 1)
            assert torch.equal(batch['weights'][:, 0], rep.weights[r * h:(r + 1) * h])
            shards.append(batch)
            idxs.append(idx_all)
        assert torch.equal(reps[0].weights, reps[1].weights)
        assert _lockstep(learners, shards) == 1
        assert _bits_equal(learners[0], learners[1])
        for rep, idx_all, l in zip(reps, idxs, learners):
            rep.update_priorities_from_td(idx_all, l.td_error)
        assert torch.equal(reps[0].tree, reps[1].tree), it
        assert torch.equal(reps[0].rng.dev, reps[1].rng.dev), it
        assert reps[0].max_priority == reps[1].max_priority
        PR.check_drawn_leaves(reps[0].tree, cap, want, learners[0].td_error.cpu().numpy())


# ---------------------------------------------------------- unchanged paths
def test_dp_none_and_world_1_are_the_plain_learner():
    lc, D, A, init, batches = R.envelope_case('b96_duel_dq')
    ec = discrete_env_config(D, A)
    plain = _load(DQNLearner(lc, ec), init)
    none = _load(DQNLearner(lc, ec, dp=None), init)
    one = _load(DQNLearner(lc, ec, dp=_Group(1, 0)), init)
    assert none.dp is None and one.dp is None
    for it, b in enumerate(batches):
        d = _dev(b)
        for l in (plain, none, one):
            l.learn(d)
        assert _bits_equal(plain, none) and _bits_equal(plain, one), it
        assert one._xbuf is None and tuple(one.td_error.shape) == (lc.replay.batch_size,)
        assert list(one._learn_phases(d)) == [] and one.current_iteration == 2 * it + 2
        plain.learn(d)
        none.learn(d)
        assert _bits_equal(plain, one), it


@pytest.mark.parametrize('cls', [UniformReplay, PrioritizedReplay])
def test_sample_shard_of_world_1_is_sample_batch(cls):
    lc, D, A, _, _ = R.envelope_case('b96_duel_dq')
    lc = copy.deepcopy(lc)
    lc.replay.memory_size, lc.replay.sampling_start_size = 128, 10
    ec = discrete_env_config(D, A)
    rows = torch.randn(100, 2 * D + 3, generator=torch.Generator().manual_seed(3))
    a, b = cls(lc, ec, seed=11), cls(lc, ec, seed=11)
    kw = {'beta': 0.4} if cls is PrioritizedReplay else {}
    for rep in (a, b):
        rep.insert_rows(rows)
    for it in range(2):
        ia, ba = a.sample_batch(32, **kw)
        ib, bb = b.sample_shard(32, 0, 1, **kw)
        assert torch.equal(ia, ib) and sorted(ba) == sorted(bb)
        for k in ba:
            assert torch.equal(ba[k].view(torch.int32), bb[k].view(torch.int32)), (it, k)
        assert torch.equal(a.rng.dev, b.rng.dev)
    before = b.rng.dev.clone()
    for bad in ((33, 0, 2), (32, 2, 2), (32, -1, 2), (32, 0, 0)):
        with pytest.raises(ValueError):
            b.sample_shard(*bad, **kw)
    assert torch.equal(before, b.rng.dev)                   # nothing was drawn
    if cls is PrioritizedReplay:
        with pytest.raises(ValueError, match='sample_shard'):
            b.sample_batch(32, world=2)
