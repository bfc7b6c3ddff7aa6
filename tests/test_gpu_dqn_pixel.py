"""DQNLearner / QAgentBatch with model.convs on uint8 frames against the CPU
restatement of tests/qconv_ref.py: learn() on the envelope bar, the raw
first-step gradient (conv layers included), hipGraph replay, the frame-shared
prioritized-replay loop, the full-state checkpoint and batched acting."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

from surreal_amd.agent import QAgentBatch
from surreal_amd.config import discrete_pixel_env_config
from surreal_amd.dqn import DQNLearner, ffq_param_names
from surreal_amd.replay import PrioritizedReplay
from tests import dqn_ref as R
from tests import parity as P
from tests import qconv_ref as Q
from tests.test_gpu_boundary import ref_checkpoint_restore, ref_checkpoint_save
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _learner(lc, shape, A, init=None, **kw):
    learner = DQNLearner(lc, discrete_pixel_env_config(shape, A), **kw)
    if init is not None:
        learner.q_func.load_state_dict(init['q_func'])
        learner.q_target.load_state_dict(init['q_target'])
    return learner


def _dev(b):
    return {k: torch.as_tensor(v).to(DEV) if k in ('obs', 'obs_next')
            else torch.as_tensor(v, dtype=torch.float32).to(DEV) for k, v in b.items()}


def _state(learner):
    return {'q_func': R.flat_of(learner.q_func.state_dict()),
            'q_target': R.flat_of(learner.q_target.state_dict())}


def _bits_equal(a, b):
    return all(torch.equal(getattr(a, n).flat, getattr(b, n).flat) for n in ('q_func', 'q_target')) \
        and torch.equal(a.td_error, b.td_error) and torch.equal(a.stats_buf, b.stats_buf)


@pytest.mark.parametrize('name', sorted(Q.PIX_CASES))
def test_pixel_learn_envelope(name):
    """3 steps, the target copy falling after the second: the bars of
    tests/dqn_ref.py::envelope_check, restated for uint8 frames"""
    lc, shape, A, init, batches = Q.pix_case(name)
    learner = _learner(lc, shape, A, init)
    assert list(learner.q_func.state_dict()) == list(init['q_func']) == ffq_param_names(
        len(lc.model.convs), len(lc.model.fc_hidden_sizes), lc.model.dueling)
    got = []
    for it, b in enumerate(batches):
        learner.learn(_dev(b) if it != 1 else b)          # (step 2 from the host: preprocess())
        got.append((_state(learner), learner.last_stats(), learner.td_error.cpu().double().numpy()))
        assert torch.equal(learner.q_func.flat, learner.q_target.flat) == (it == 1)
    assert learner.target_update_tracker.value == 3 * lc.replay.batch_size
    P.print_report(Q.envelope_check_pixels(lc, shape, A, init, batches, got))


@pytest.mark.parametrize('name', ['pix_small', 'pix_plain'])
def test_pixel_first_step_gradient(name):
    """the raw gradient image of the first step against autograd of the fp32 /
    fp64 reference, parameter by parameter, conv layers included; `mag` is the
    largest sum of |terms| of one output"""
    lc, shape, A, init, batches = Q.pix_case(name)
    learner = _learner(lc, shape, A, init)
    b = batches[0]
    learner.learn(_dev(b))
    g = learner.opt['g'].cpu()
    refs = {}
    for dt in (torch.float32, torch.float64):
        ref = Q.PixLearnerRef(lc, shape, A, dt)
        ref.load(init)
        ref.q_func.trace = []
        ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'], b.get('weights'),
                     step=False)
        refs[dt] = ref
    r32, r64 = refs[torch.float32], refs[torch.float64]
    mags = {}
    for lin, x, z in r64.q_func.trace:
        dz = z.grad.abs()
        if isinstance(lin, nn.Conv2d):
            mags[lin.weight] = float(torch.nn.grad.conv2d_weight(
                x.detach().abs(), lin.weight.shape, dz, stride=lin.stride, padding=lin.padding).max())
            mags[lin.bias] = float(dz.sum(dim=(0, 2, 3)).max())
        else:
            mags[lin.weight] = float((dz.t() @ x.detach().abs()).max())
            mags[lin.bias] = float(dz.sum(0).max())
    p32 = dict(r32.q_func.named_parameters())
    p64 = dict(r64.q_func.named_parameters())
    seen = 0
    for pname, p in learner.q_func.named_parameters():
        off = learner.q_func.off(p)
        mine = g[off:off + p.numel()].view(p.shape)
        _fp32_as_good_as_torch(mine, p32[pname].grad, p64[pname].grad, 4e-6, mag=mags[p64[pname]])
        seen += p.numel()
    assert seen == g.numel()


def test_pixel_graph_replay_bit_exact():
    """use_graph=True over static inputs that include the uint8 frames:
    bit-identical to eager over 4 steps"""
    lc, shape, A, init, _ = Q.pix_case('pix_small')
    B = lc.replay.batch_size
    eager, graph = _learner(lc, shape, A, init), _learner(lc, shape, A, init, use_graph=True)
    for it, b in enumerate(Q.pix_batches(B, shape, A, 3, True, steps=4)):
        d = _dev(b)
        eager.learn(d)
        graph.learn(d)
        torch.cuda.synchronize()
        assert _bits_equal(eager, graph), it
        assert eager.last_stats() == graph.last_stats()
    assert graph._graph is not None and eager._graph is None
    assert graph.graph_inputs()['obs'].dtype == torch.uint8


def test_frame_shared_prioritized_replay_loop():
    """PrioritizedReplay with share_frames and frame_stacks = 4: insert,
    sample_batch, learn on its output as it is, update_priorities_from_td; a
    second learner given the same batch from the host lands on the same bits"""
    lc, shape, A, init, _ = Q.pix_case('pix_small')
    lc = copy.deepcopy(lc)
    lc.replay.memory_size, lc.replay.sampling_start_size, lc.replay.share_frames = 64, 10, True
    ec = discrete_pixel_env_config((1,) + shape[1:], A, frame_stacks=4)
    assert tuple(ec.obs_spec['pixel']['camera0']) == shape
    rep = PrioritizedReplay(lc, ec, seed=77)
    assert rep.share_frames and rep.frame_stacks == 4 and rep.width == 3
    n, B = 40, lc.replay.batch_size
    g = torch.Generator().manual_seed(4)
    rows = torch.zeros(n, 3)
    rows[:, 0] = torch.randint(0, A, (n,), generator=g).float()
    rows[:, 1] = 1.5 * torch.randn(n, generator=g)
    rows[:, 2] = (torch.rand(n, generator=g) < 0.2).float()
    # one episode: obs i stacks camera frames i..i+3, obs_next i frames i+1..i+4,
    # so the store holds n + 4 frames for 2 * 4 * n frame references
    film = torch.randint(0, 256, (n + 4,) + shape[1:], generator=g, dtype=torch.uint8)
    pix = torch.stack([film[i:i + 4] for i in range(n)])
    pix_next = torch.stack([film[i + 1:i + 5] for i in range(n)])
    rep.insert_rows(rows, pix, pix_next)
    assert rep.frames_in_use == n + 4
    la = DQNLearner(lc, ec)
    lb = DQNLearner(lc, ec)
    for l in (la, lb):
        l.q_func.load_state_dict(init['q_func'])
        l.q_target.load_state_dict(init['q_target'])
    cap = rep.capacity
    for it in range(2):
        idx, batch = rep.sample_batch(B, beta=0.4)
        frames = batch['obs']['pixel']['camera0']
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (B,) + shape
        want = idx.cpu()
        assert torch.equal(frames.cpu(), pix[want]) and \
            torch.equal(batch['obs_next']['pixel']['camera0'].cpu(), pix_next[want])
        la.learn(batch)
        host = {'obs': {'pixel': {'camera0': pix[want].numpy()}},
                'obs_next': {'pixel': {'camera0': pix_next[want].numpy()}},
                'actions': rows[want, 0:1].numpy().astype(np.int32),
                'rewards': rows[want, 1:2].numpy(), 'dones': rows[want, 2:3].numpy(),
                'weights': batch['weights'].cpu().numpy()}
        lb.learn(host)
        assert _bits_equal(la, lb), it
        rep.update_priorities_from_td(idx, la.td_error)
        td = la.td_error.cpu().numpy()
        leaves = rep.tree.cpu().numpy()[2 * cap::2]
        last = {int(s): (abs(float(t)) + 1e-6) ** 0.6 for s, t in zip(want.tolist(), td)}
        slots = np.array(sorted(last))
        exp = np.array([last[s] for s in slots])
        assert (np.abs(leaves[slots] - exp) / exp <= 2.0 ** -51).all()


def test_pixel_checkpoint_full_state():
    lc, shape, A, init, _ = Q.pix_case('pix_small')
    bs = [_dev(b) for b in Q.pix_batches(lc.replay.batch_size, shape, A, 8, True, steps=4)]
    l1 = _learner(lc, shape, A, init, checkpoint_full_state=True)
    for b in bs[:2]:
        l1.learn(b)
    blob = ref_checkpoint_save(l1)
    l2 = _learner(lc, shape, A, None, seed=5, checkpoint_full_state=True)
    assert not torch.equal(l1.q_func.flat, l2.q_func.flat)
    ref_checkpoint_restore(l2, blob)
    assert l2.current_iteration == 2 and l2.target_update_tracker.value == 2 * lc.replay.batch_size
    for b in bs[2:]:
        l1.learn(b)
        l2.learn(b)
        assert _bits_equal(l1, l2)
    for k in ('m', 'v', 'step'):
        assert torch.equal(l1.opt[k], l2.opt[k])


@pytest.mark.parametrize('mode', ['training', 'eval_deterministic'])
def test_q_agent_batch_on_frames(mode):
    """5 agents on uint8 frames against 5 sequential reference agents under the
    same random.seed: the same actions and the same state of `random`"""
    lc, shape, A, init, _ = Q.pix_case('pix_small')
    lc.algo.exploration.steps, lc.algo.exploration.final_eps, lc.eval.eps = 100, 0.1, 0.3
    n, T0 = 5, [0, 50, 99, 5000, 7]
    ec = discrete_pixel_env_config(shape, A)
    batch = QAgentBatch(lc, ec, n, agent_mode=mode)
    batch.q_func.load_state_dict(init['q_func'])
    batch.T[:] = T0
    refs = []
    for t in T0:
        r = Q.QAgentPixRef(lc, shape, A, mode)
        r.q_func.load_state_dict(init['q_func'])
        r.T = t
        refs.append(r)
    q64 = Q.QConvRef(shape, A, lc.model.convs, lc.model.fc_hidden_sizes, lc.model.dueling, True,
                     torch.float64)
    q64.load_state_dict({k: v.double() for k, v in init['q_func'].items()})
    g = torch.Generator().manual_seed(12)
    for rnd in range(3):
        obs = torch.randint(0, 256, (n,) + shape, generator=g, dtype=torch.uint8)
        with torch.no_grad():
            top = q64(obs.double()).sort(1).values
        assert float((top[:, -1] - top[:, -2]).min()) >= 1e-4 * float(top.abs().max())
        random.seed(100 + rnd)
        want = [r.act(obs[i].numpy()) for i, r in enumerate(refs)]
        state = random.getstate()
        random.seed(100 + rnd)
        got = batch.act({'pixel': {'camera0': obs.numpy()}} if rnd else obs.numpy())
        assert got.tolist() == want, (rnd, got, want)
        assert random.getstate() == state
    assert batch.T.tolist() == [t + 3 for t in T0]
