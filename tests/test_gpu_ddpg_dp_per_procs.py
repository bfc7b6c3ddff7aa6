"""Data-parallel DDPG with a prioritized replay over the real exchange: two
processes share cuda:0 and all-reduce over torch.distributed (gloo: RCCL
refuses two ranks on one GPU; a multi-GPU node runs the same code over 'nccl')
through learner.TorchDistAllReduce.  Each rank holds a PrioritizedReplay
replica (same seed, same inserts), constructs its TD3 learner from a different
seed (the constructor's broadcast replicates rank 0's weights) and runs
sample_shard -> learn -> update_priorities_from_td(idx_all, td_error) for 3
steps.  Required: the ranks end bit-identical (draws, weights, parameters,
targets, statistics, TD errors and the priority trees), and rank 0's states are
bit-equal to the one-process _lockstep simulation of the same case
(tests/test_gpu_ddpg_dp_per.py), whose rank 0 that file holds to the envelope."""
import numpy as np
import pytest
import torch

from tests.dp_harness import Group, spawn_ranks
from tests.helpers import per_cfg, replay_rows

pytestmark = pytest.mark.gpu

BG, D, A, NROWS, SEED, STEPS, BETA, WORLD = 96, 17, 6, 150, 4321, 3, 0.4, 2


def _cfg(B):
    return per_cfg(B, 200, double=True, action_reg=True)


def _replica():
    from surreal_amd.config import gym_env_config
    from surreal_amd.replay import PrioritizedReplay
    rep = PrioritizedReplay(_cfg(BG // WORLD), gym_env_config(D, A), seed=SEED, device='cuda:0')
    rep.insert_rows(replay_rows(NROWS, D, A, 3))
    return rep


def _record(rep, idx_all, learner):
    from tests.test_gpu_ddpg import _ddpg_state
    return {'idx': idx_all.cpu().clone(), 'weights': rep.weights.cpu().clone(),
            'state': _ddpg_state(learner), 'stats_buf': learner.stats_buf.cpu().clone(),
            'td': learner.td_error.cpu().clone(), 'tree': rep.tree.cpu().clone()}


def _worker(rank, world):
    from surreal_amd.config import gym_env_config
    from surreal_amd.ddpg import DDPGLearner
    from surreal_amd.learner import TorchDistAllReduce
    rep = _replica()
    # a different seed per rank: the constructor's broadcast replicates rank 0's weights
    learner = DDPGLearner(_cfg(BG // world), gym_env_config(D, A), seed=5 + rank, device='cuda:0',
                          dp=TorchDistAllReduce())
    res = []
    for it in range(STEPS):
        idx_all, batch = rep.sample_shard(BG, rank, world, beta=BETA)
        np.random.seed(100 + it)                    # the TD3 smoothing noise's stream
        learner.learn(batch)
        rep.update_priorities_from_td(idx_all, learner.td_error, eps=1e-6)
        res.append(_record(rep, idx_all, learner))
    return res


def _simulate():
    """the same case with both ranks in this process (rank 0's constructor seed)"""
    from surreal_amd.config import gym_env_config
    from surreal_amd.ddpg import DDPGLearner
    from tests.test_gpu_ddpg_dp_per import _step
    reps = [_replica() for _ in range(WORLD)]
    learners = [DDPGLearner(_cfg(BG // WORLD), gym_env_config(D, A), seed=5, device='cuda:0',
                            dp=Group(WORLD, r)) for r in range(WORLD)]
    res = []
    for it in range(STEPS):
        draws = [rep.sample_shard(BG, r, WORLD, beta=BETA) for r, rep in enumerate(reps)]
        assert _step(learners, [b for _, b in draws], 100 + it) == 2
        for rep, (idx_all, _), l in zip(reps, draws, learners):
            rep.update_priorities_from_td(idx_all, l.td_error, eps=1e-6)
        res.append(_record(reps[0], draws[0][0], learners[0]))
    return res


def _assert_records_equal(a, b, tag):
    for k in ('idx', 'weights', 'stats_buf', 'td', 'tree'):
        assert torch.equal(a[k], b[k]), (tag, k)
    assert sorted(a['state']) == sorted(b['state'])
    for k in a['state']:
        assert torch.equal(a['state'][k], b['state'][k]), (tag, k)


@pytest.mark.timeout(600)
def test_two_process_ddpg_dp_per_matches_the_lockstep_simulation():
    out = spawn_ranks(_worker, WORLD)
    sim = _simulate()
    for it in range(STEPS):
        r0, r1 = out[0][it], out[1][it]
        assert tuple(r0['td'].shape) == (BG,) and {'critic2', 'critic2_t'} <= set(r0['state'])
        _assert_records_equal(r0, r1, ('ranks', it))
        _assert_records_equal(r0, sim[it], ('lockstep', it))
    assert not torch.equal(out[0][0]['td'], out[0][1]['td'])
