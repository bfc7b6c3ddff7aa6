"""DQNLearner / QAgentBatch (surreal_amd/dqn.py, agent.py) against the CPU
restatement of tests/dqn_ref.py: the learn() step on the project's envelope
bar, the raw first-step gradient, the batch forms learn() takes, hipGraph
replay, the prioritized-replay loop, the full-state checkpoint and batched
epsilon-greedy acting."""
import random

import numpy as np
import pytest
import torch

from surreal_amd.agent import QAgentBatch
from surreal_amd.aggregator import SSARAggregator
from surreal_amd.config import discrete_env_config
from surreal_amd.dqn import DQNLearner
from surreal_amd.replay import PrioritizedReplay
from tests import dqn_ref as R
from tests import parity as P
from tests import per_ref as PR
from tests.test_gpu_boundary import ref_checkpoint_restore, ref_checkpoint_save
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _learner(lc, D, A, init=None, **kw):
    learner = DQNLearner(lc, discrete_env_config(D, A), **kw)
    if init is not None:
        learner.q_func.load_state_dict(init['q_func'])
        learner.q_target.load_state_dict(init['q_target'])
    return learner


def _dev(b):
    return {k: torch.as_tensor(v, dtype=torch.float32).to(DEV) for k, v in b.items()}


def _state(learner):
    return {'q_func': R.flat_of(learner.q_func.state_dict()),
            'q_target': R.flat_of(learner.q_target.state_dict())}


def _bits_equal(a, b):
    return all(torch.equal(getattr(a, n).flat, getattr(b, n).flat) for n in ('q_func', 'q_target')) \
        and torch.equal(a.td_error, b.td_error) and torch.equal(a.stats_buf, b.stats_buf)


# --------------------------------------------------- learn() on the envelope
@pytest.mark.parametrize('name', sorted(R.ENVELOPE_CASES))
def test_dqn_learn_envelope(name):
    """3 steps, the target copy falling after the second
    (target_network_update_freq = 2 B): q_func, q_target and td_error within
    2 x envelope + 1e-6 of scale of the fp64 reference, the statistics within
    max(2 w + 1e-6, 1e-5) (tests/dqn_ref.py envelope_check)."""
    lc, D, A, init, batches = R.envelope_case(name)
    learner = _learner(lc, D, A, init)
    assert list(learner.q_func.state_dict()) == list(init['q_func'])
    got = []
    for b in batches:
        learner.learn(_dev(b))
        got.append((_state(learner), learner.last_stats(), learner.td_error.cpu().double().numpy()))
    assert learner.target_update_tracker.value == 3 * lc.replay.batch_size
    assert learner.module_dict()['q_func'] is learner.q_func
    P.print_report(R.envelope_check(lc, D, A, init, batches, got))


@pytest.mark.parametrize('name', ['b96_duel_dq', 'b96_plain', 'three_hidden'])
def test_first_step_gradient(name):
    """the raw gradient image of the first step (before clip and Adam) against
    autograd of the fp32 / fp64 reference, parameter by parameter -- the
    stacked first layer's rows of both streams included; `mag` is the largest
    sum of |terms| of one output (|dz|^T |x|, column sums of |dz|)."""
    lc, D, A, init, batches = R.envelope_case(name)
    learner = _learner(lc, D, A, init)
    b = batches[0]
    learner.learn(_dev(b))
    g = learner.opt['g'].cpu()
    refs = {}
    for dt in (torch.float32, torch.float64):
        ref = R.DQNLearnerRef(lc, D, A, dt)
        ref.load(init)
        ref.q_func.trace = []
        ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'], b.get('weights'),
                     step=False)
        refs[dt] = ref
    r32, r64 = refs[torch.float32], refs[torch.float64]
    mags = {}
    for lin, x, z in r64.q_func.trace:
        dz = z.grad.abs()
        mags[lin.weight] = float((dz.t() @ x.detach().abs()).max())
        mags[lin.bias] = float(dz.sum(0).max())
    p32 = dict(r32.q_func.named_parameters())
    seen = 0
    for pname, p in learner.q_func.named_parameters():
        off = learner.q_func.off(p)
        mine = g[off:off + p.numel()].view(p.shape)
        p64 = dict(r64.q_func.named_parameters())[pname]
        _fp32_as_good_as_torch(mine, p32[pname].grad, p64.grad, mag=mags[p64])
        seen += p.numel()
    assert seen == g.numel()


# -------------------------------------------------------------- batch forms
def test_learn_on_replay_column_views_and_host_batches():
    """column views of a replay rows tensor (strides honoured, nothing copied)
    give the bits of contiguous copies; a host batch from SSARAggregator (int32
    actions) through preprocess() gives the bits of the device batch"""
    lc, D, A, init, _ = R.envelope_case('b96_duel_dq')
    B = lc.replay.batch_size
    g = torch.Generator().manual_seed(9)
    exps = []
    for i in range(B):
        o0, o1 = torch.randn(D, generator=g).numpy(), torch.randn(D, generator=g).numpy()
        a = int(torch.randint(0, A, (1,), generator=g))
        exps.append({'obs': [{'low_dim': {'flat_inputs': o0}}, {'low_dim': {'flat_inputs': o1}}],
                     'action': np.int64(a) if i % 2 else a, 'reward': float(torch.randn(1, generator=g)),
                     'done': bool(i % 5 == 0)})
    ec = discrete_env_config(D, A)
    rep = PrioritizedReplay(_per_cfg(lc, 128), ec, seed=0)
    assert rep.act_dim == 1 and rep.width == 2 * D + 3
    rows = torch.as_tensor(rep.pack(exps)).to(DEV)
    views = rep.split(rows)
    assert views['actions'].stride(0) == rep.width and not views['obs_next'].is_contiguous()
    assert views['actions'].data_ptr() == rows.data_ptr() + 4 * D
    la, lb, lc_ = (_learner(lc, D, A, init) for _ in range(3))
    host = SSARAggregator(ec.obs_spec, ec.action_spec).aggregate(exps)
    assert host['actions'].dtype == np.int32
    assert np.array_equal(host['actions'].reshape(-1), rows[:, D].cpu().numpy())
    for it in range(2):
        la.learn(views)
        lb.learn({k: v.contiguous() for k, v in views.items()})
        lc_.learn(host)
        assert _bits_equal(la, lb) and _bits_equal(lb, lc_), it
    bad = dict(host, actions=np.full((B,), A, dtype=np.int32))
    before = lc_.q_func.flat.clone()
    with pytest.raises(ValueError, match='actions'):
        lc_.learn(bad)
    assert torch.equal(before, lc_.q_func.flat)


# ------------------------------------------------------------------- graph
@pytest.mark.parametrize('weights', [True, False])
def test_dqn_graph_replay_bit_exact(weights):
    """use_graph=True replays the eager launch sequence over static inputs:
    bit-identical over 4 steps, the target copies (after steps 2 and 4) on the
    host between replays"""
    lc, D, A, init, _ = R.envelope_case('b512')
    B = lc.replay.batch_size
    eager, graph = _learner(lc, D, A, init), _learner(lc, D, A, init, use_graph=True)
    for it, b in enumerate(R.dqn_batches(B, D, A, 3, weights, steps=4)):
        d = _dev(b)
        eager.learn(d)
        graph.learn(d)
        torch.cuda.synchronize()
        assert _bits_equal(eager, graph), it
        assert eager.last_stats() == graph.last_stats()
        same = torch.equal(graph.q_func.flat, graph.q_target.flat)
        assert same == (it in (1, 3)), it
    assert graph._graph is not None and eager._graph is None


# ---------------------------------------------------------------- PER loop
def _per_cfg(lc, memory):
    import copy
    lc = copy.deepcopy(lc)
    lc.replay.memory_size = memory
    lc.replay.sampling_start_size = 10
    return lc


def test_prioritized_replay_loop():
    """sample_batch(64, beta 0.4) -> learn -> update_priorities_from_td on a
    discrete-action replay of 300 transitions: the drawn indices are
    tests/per_ref.py's, the leaves of the drawn slots are (|td| + 1e-6) ** 0.6
    (fp64, from learner.td_error; a repeated slot keeps its last), and
    max_priority follows.  The leaf is the device's fp64 pow and the expected
    value the host's, two different libraries each within one unit in the last
    place of the true power, so "equal" is held to 2 ulp = 2^-51 relative
    (bit equality does not hold: the largest difference seen is 2.2e-16, one
    ulp); test_gpu_per.py pins the same kernel at alpha * 2^-24."""
    lc, D, A, init, _ = R.envelope_case('b96_duel_dq')
    lc = _per_cfg(lc, 400)
    ec, seed, n, B = discrete_env_config(D, A), 2468, 300, 64
    rep = PrioritizedReplay(lc, ec, seed=seed)
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(n, rep.width, generator=g)
    rows[:, D] = torch.randint(0, A, (n,), generator=g).float()
    rows[:, 2 * D + 2] = (torch.rand(n, generator=g) < 0.1).float()
    rep.insert_rows(rows)
    cap = rep.capacity
    learner = _learner(lc, D, A, init)
    random.seed(seed)
    top = 1.0
    for it in range(2):
        want, _ = PR.ref_from_device(rep.tree, cap)[0].sample(n, B, 0.4)
        idx, batch = rep.sample_batch(B, beta=0.4)
        assert idx.cpu().tolist() == want, it
        learner.learn(batch)
        rep.update_priorities_from_td(idx, learner.td_error)
        td = learner.td_error.cpu().numpy()
        PR.check_drawn_leaves(rep.tree, cap, want, td)
        top = max(top, float(np.abs(td.astype(np.float64)).max()) + 1e-6)
        assert rep.max_priority == top


# -------------------------------------------------------------- checkpoint
def test_dqn_checkpoint_full_state():
    """save after 2 steps (the target copy has just happened), restore into a
    fresh learner, 2 more steps: the bits of 4 uninterrupted steps, the tracker
    value included (the second copy falls after step 4)"""
    lc, D, A, init, _ = R.envelope_case('b96_duel_dq')
    bs = [_dev(b) for b in R.dqn_batches(lc.replay.batch_size, D, A, 8, True, steps=4)]
    l1 = _learner(lc, D, A, init, checkpoint_full_state=True)
    for b in bs[:2]:
        l1.learn(b)
    blob = ref_checkpoint_save(l1)
    l2 = DQNLearner(lc, discrete_env_config(D, A), seed=5, checkpoint_full_state=True)
    assert not torch.equal(l1.q_func.flat, l2.q_func.flat)
    ref_checkpoint_restore(l2, blob)
    assert l2.current_iteration == 2 and l2.target_update_tracker.value == 2 * lc.replay.batch_size
    for b in bs[2:]:
        l1.learn(b)
        l2.learn(b)
        assert _bits_equal(l1, l2)
    assert torch.equal(l2.q_func.flat, l2.q_target.flat)
    for k in ('m', 'v', 'step'):
        assert torch.equal(l1.opt[k], l2.opt[k])


# ------------------------------------------------------------------ agents
@pytest.mark.parametrize('mode', ['training', 'eval_stochastic', 'eval_deterministic'])
def test_q_agent_batch_matches_sequential_agents(mode):
    """7 agents at different step counts against 7 sequential QAgentRef under
    the same random.seed: the same actions over 3 rounds and the same state of
    `random` afterwards.  Observations are kept whose fp64 arg-max margin is at
    least 1e-4 of the largest score, so fp32 rounding cannot change a greedy
    action."""
    lc, D, A, init, _ = R.envelope_case('b96_duel_dq')
    lc.algo.exploration.steps, lc.algo.exploration.final_eps, lc.eval.eps = 100, 0.1, 0.3
    n, T0 = 7, [0, 3, 50, 99, 100, 5000, 7]
    learner = _learner(lc, D, A, init)
    batch = QAgentBatch(lc, discrete_env_config(D, A), n, agent_mode=mode)
    batch.load_module_dict(learner.module_dict())
    batch.T[:] = T0
    refs = []
    for t in T0:
        r = R.QAgentRef(lc, D, A, mode)
        r.q_func.load_state_dict(init['q_func'])
        r.T = t
        refs.append(r)
    q64 = R.FFQfuncRef(D, A, lc.model.fc_hidden_sizes, lc.model.dueling, torch.float64)
    q64.load_state_dict({k: v.double() for k, v in init['q_func'].items()})
    g = torch.Generator().manual_seed(12)
    greedy_seen = 0
    for rnd in range(3):
        obs = torch.randn(n, D, generator=g)
        with torch.no_grad():
            top = q64(obs.double()).sort(1).values
        assert float((top[:, -1] - top[:, -2]).min()) >= 1e-4 * float(top.abs().max())
        random.seed(100 + rnd)
        want = [r.act(obs[i].numpy()) for i, r in enumerate(refs)]
        state = random.getstate()
        random.seed(100 + rnd)
        got = batch.act(obs.numpy())
        assert got.tolist() == want, (rnd, got, want)
        assert random.getstate() == state
        with torch.no_grad():
            greedy_seen += sum(int(a == int(q64(obs[i:i + 1].double()).argmax())) for i, a in enumerate(want))
    assert batch.T.tolist() == [t + 3 for t in T0]
    assert greedy_seen >= (21 if mode == 'eval_deterministic' else 1)
    # the published numpy form loads too
    batch.load_numpy({'q_func': {k: v.cpu().numpy() for k, v in learner.q_func.state_dict().items()}})
