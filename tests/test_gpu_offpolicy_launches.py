"""The library launches of the off-policy learners and the replay draws, by
entry-point name and in order, against tests/golden/offpolicy_launches.json
(this project's own record, taken before the learn() frame, the exchange image
and the draw path were each given one home): a refactor of the host side must
leave every sequence as it is.  surreal_amd._lib.call is wrapped; nothing else
about a case is special."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

from surreal_amd import _lib
from surreal_amd import synthetic
from surreal_amd.config import discrete_env_config, gym_env_config, pixel_env_config
from surreal_amd.ddpg import DDPGLearner
from surreal_amd.dqn import DQNLearner
from surreal_amd.replay import PrioritizedReplay, UniformReplay
from tests import dqn_ref
from tests.dp_harness import Group, cut, lockstep, to_dev
from tests.helpers import per_cfg, replay_rows

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'offpolicy_launches.json')


class Recorder(object):
    """_lib.call with the entry-point names kept"""

    def __init__(self):
        self.names, self._call = [], _lib.call

    def __enter__(self):
        def call(name, *args):
            self.names.append(name)
            return self._call(name, *args)
        _lib.call = call
        return self.names

    def __exit__(self, *exc):
        _lib.call = self._call


# ------------------------------------------------------------------ learners
def _dqn(name, world):
    lc, D, A, init, batches = dqn_ref.envelope_case(name)
    lc = copy.deepcopy(lc)
    lc.replay.batch_size //= world
    learners = [DQNLearner(lc, discrete_env_config(D, A), dp=Group(world, r)) for r in range(world)]
    for l in learners:
        l.q_func.load_state_dict(init['q_func'])
        l.q_target.load_state_dict(init['q_target'])
    return learners, to_dev(batches[0])


def _ddpg(B, world, weights, **kw):
    D, A = 17, 6
    learners = [DDPGLearner(per_cfg(B // world, 200, **kw), gym_env_config(D, A), seed=2,
                            dp=Group(world, r)) for r in range(world)]
    batch = to_dev({k: v.numpy() for k, v in synthetic.ddpg_batch(B, D, A, seed=1).items()})
    if weights:
        batch['weights'] = torch.rand(B, 1, generator=torch.Generator().manual_seed(3)).cuda() + 0.05
    return learners, batch


def _learn(learners, batch):
    world = len(learners)
    n = batch['actions'].shape[0] // world
    with Recorder() as names:
        if world == 1:
            learners[0].learn(batch)
        else:
            lockstep(learners, [cut(batch, r, n) for r in range(world)])
        torch.cuda.synchronize()
    return names


LEARN = {}
for _name in ('b96_duel_dq', 'b96_plain'):
    for _world in (1, 2):
        LEARN[f'dqn-{_name}-world{_world}'] = functools.partial(_dqn, _name, _world)
for _w, _tag in ((False, 'plain'), (True, 'weights')):
    LEARN[f'ddpg-b96-world1-{_tag}'] = functools.partial(_ddpg, 96, 1, _w)
    LEARN[f'ddpg-td3-b96-world2-{_tag}'] = functools.partial(_ddpg, 96, 2, _w, double=True,
                                                              action_reg=True)


def record_learn(case):
    np.random.seed(100)                                  # the TD3 smoothing noise's stream
    return _learn(*LEARN[case]())


# -------------------------------------------------------------------- replay
def _replay(cls, mode):
    """a filled replay in one of the three storage modes, and its batch size"""
    D, A, cam, B, mem, n = 5, 2, (9, 20, 20), 16, 40, 20
    lc = per_cfg(B, mem)
    if mode == 'low_dim':
        rep = cls(lc, gym_env_config(D, A), seed=5)
        rep.insert_rows(replay_rows(n, D, A, 3))
        return rep, B
    ec = pixel_env_config(D, A, cam)
    if mode == 'shared':
        ec['frame_stacks'] = 3
        lc.replay.share_frames, lc.replay.frame_slots = True, 4 * mem
    g = torch.Generator().manual_seed(7)
    pix = torch.randint(0, 256, (n,) + cam, generator=g, dtype=torch.uint8)
    pix_next = torch.randint(0, 256, (n,) + cam, generator=g, dtype=torch.uint8)
    rep = cls(lc, ec, seed=5)
    rep.insert_rows(replay_rows(n, D, A, 3), pix, pix_next)
    assert rep.share_frames == (mode == 'shared')
    return rep, B


REPLAY = {f'{cls.__name__}-{mode}': (cls, mode) for cls in (UniformReplay, PrioritizedReplay)
          for mode in ('low_dim', 'pixel', 'shared')}


def record_replay(case):
    """sample, sample_batch, sample_shard(world 2), and sample_batch again (its
    buffers are of another row count after the shard); a call the mode refuses
    is recorded by its exception's name"""
    cls, mode = REPLAY[case]
    rep, B = _replay(cls, mode)
    kw = {'beta': 0.4} if cls is PrioritizedReplay else {}
    out = {}
    for step, draw in (('sample', lambda: rep.sample(B, **kw)),
                       ('sample_batch', lambda: rep.sample_batch(B, **kw)),
                       ('sample_shard', lambda: rep.sample_shard(B, 1, 2, **kw)),
                       ('sample_batch_again', lambda: rep.sample_batch(B, **kw))):
        with Recorder() as names:
            try:
                draw()
            except ValueError as e:
                names.append(type(e).__name__)
            torch.cuda.synchronize()
        out[step] = names
    return out


def record(case):
    return record_learn(case) if case in LEARN else record_replay(case)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_names_these_cases(golden):
    assert sorted(golden) == sorted(list(LEARN) + list(REPLAY))


@pytest.mark.parametrize('case', list(LEARN) + list(REPLAY))
def test_launch_sequence_is_the_recorded_one(case, golden):
    got = record(case)
    assert got, case
    assert got == golden[case]
