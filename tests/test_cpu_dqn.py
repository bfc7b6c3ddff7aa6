"""DQN, host side (no GPU): the test-side reference against hand-derived
closed forms, the power of the envelope check the GPU test relies on, the
conditions its batches must meet, configuration errors, the host-side target
counter and the agent's draw order."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

from surreal_amd.config import (DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config,
                                gym_env_config, pixel_env_config)
from surreal_amd.dqn import TargetUpdateTracker, dqn_specs
from tests import dqn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dqn_known_answers.json')


# ------------------------------------------------------------ closed form
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_reference_known_answers(dtype):
    """tests/golden/make_dqn_golden.py: a terminal row with |td| > 1 and a row
    with |td| < 1 whose double-Q action differs from the target's own maximum.
    Every intermediate is a dyadic rational, so fp32 is exact up to the 1/3 of
    the dueling gradient."""
    with open(GOLDEN) as f:
        k = json.load(f)
    lc = R.dqn_config(2, k['hidden'])
    lc.algo.gamma = k['gamma']
    lc.algo.grad_norm_clipping = None
    ref = R.DQNLearnerRef(lc, k['D'], k['A'], dtype)
    ref.load({n: {p: torch.tensor(v) for p, v in k[n].items()} for n in ('q_func', 'q_target')})
    stats, td = ref.optimize(k['obs'], k['actions'], k['rewards'], k['obs_next'], k['dones'],
                             k['weights'], step=False)
    tol = 1e-12 if dtype == torch.float64 else 1e-6
    assert np.allclose(ref.last['y'].double().numpy(), k['y'], rtol=0, atol=tol)
    assert np.allclose(td.double().numpy(), k['td'], rtol=0, atol=tol)
    assert abs(stats['loss'] - k['loss']) <= tol and abs(stats['td_error'] - k['td_error']) <= tol
    ts = ref.last['target_scores'].double().numpy()
    assert abs(ts[1].max() - k['target_own_max'][1]) <= tol and int(ts[1].argmax()) == 0
    assert int(ref.last['scanned'][1].argmax()) == 2 and abs(ts[1, 2] - k['double_q_value'][1]) <= tol
    ga = ref.q_func.fc_action_layers[-1].bias.grad.double().numpy()
    gv = ref.q_func.fc_state_layers[-1].bias.grad.double().numpy()
    assert np.allclose(ga, k['grad_action_bias'], rtol=0, atol=tol)
    assert np.allclose(gv, k['grad_state_bias'], rtol=0, atol=tol)


def test_golden_file_matches_its_generator():
    from tests.golden import make_dqn_golden as G
    with open(GOLDEN) as f:
        assert json.load(f) == json.loads(json.dumps(G.case()))


# ------------------------------------------- the envelope check can fail
CHECKER_CASE = 'b96_duel_dq'
# fault -> the envelope entries it must fail
FAULT_FAILS = {'target_argmax': ('td_error@0',), 'no_mean': ('td_error@0',),
               'no_dones': ('td_error@0',), 'no_clamp': ('q_func@0',),
               'no_weights': ('q_func@0', 'stat:loss@0')}


@pytest.fixture(scope='module')
def checker_case():
    return R.envelope_case(CHECKER_CASE)


def test_unfaulted_fp32_reference_passes_the_envelope(checker_case):
    lc, D, A, init, batches = checker_case
    report = R.envelope_check(lc, D, A, init, batches, R.run_reference(lc, D, A, init, batches))
    assert '_fail' not in report, report['_fail']


@pytest.mark.parametrize('fault', R.FAULTS)
def test_faulted_reference_fails_the_envelope(checker_case, fault):
    lc, D, A, init, batches = checker_case
    got = R.run_reference(lc, D, A, init, batches, fault=fault)
    report = R.envelope_check(lc, D, A, init, batches, got)
    for name in FAULT_FAILS[fault]:
        assert name in report.get('_fail', []), (fault, name, report.get(name))


def _fp64_steps(name):
    """per step of the fp64 reference: (batch, td, scores the arg-max scanned,
    target scores) """
    lc, D, A, init, batches = R.envelope_case(name)
    ref = R.DQNLearnerRef(lc, D, A, torch.float64)
    ref.load(init)
    out = []
    for b in batches:
        ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'], b.get('weights'))
        out.append((b, ref.last['td'].numpy(), ref.last['scanned'].numpy(),
                    ref.last['target_scores'].numpy()))
    return out


def test_checker_batches_hold_what_the_faults_need():
    """terminal rows, TD errors on both sides of 1, non-constant weights, rows
    whose online and target arg-max differ, in every step -- except that the
    third step starts right after the target copy, where the two networks are
    the same and no arg-max can differ"""
    for it, (b, td, scanned, target) in enumerate(_fp64_steps(CHECKER_CASE)):
        d = b['dones'].reshape(-1)
        assert 0 < d.sum() < d.size
        assert (np.abs(td) > 1).sum() >= 5 and (np.abs(td) < 1).sum() >= 5
        assert (np.abs(td[d == 1]) > 0).all()
        assert b['weights'].max() - b['weights'].min() > 0.3
        differ = scanned.argmax(1) != target.argmax(1)
        assert (differ & (d == 0)).sum() >= (5 if it < 2 else 0)


@pytest.mark.parametrize('name', sorted(R.ENVELOPE_CASES))
def test_argmax_margin_on_every_row(name):
    """the gap between the largest and the second-largest score the arg-max
    scans is at least 1e-5 x max|score| (about 100 fp32 roundings) on every row
    of every step, so no equally valid fp32 execution picks another action: a
    condition on the inputs, met by the choice of seed"""
    for it, (b, td, scanned, target) in enumerate(_fp64_steps(name)):
        top = np.sort(scanned, axis=1)
        gap = top[:, -1] - top[:, -2]
        assert gap.min() >= 1e-5 * np.abs(scanned).max(), (name, it, gap.min())


# ------------------------------------------------------------ config errors
def test_out_of_scope_configurations_raise():
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    ec = discrete_env_config(5, 3)
    assert dqn_specs(lc, ec) == (5, 3, [128, 128], True)
    bad = copy.deepcopy(lc)
    bad.model.convs = [[16, 8, 4]]
    with pytest.raises(ConfigError, match='convs'):
        dqn_specs(bad, ec)
    pix = pixel_env_config(5, 3)
    pix.action_spec = {'dim': (3,), 'type': 'discrete'}
    with pytest.raises(ConfigError, match='pixel'):
        dqn_specs(lc, pix)
    with pytest.raises(ConfigError, match='discrete'):
        dqn_specs(lc, gym_env_config(5, 3))
    for hs in ([], [8, 8, 8, 8]):
        bad = copy.deepcopy(lc)
        bad.model.fc_hidden_sizes = hs
        with pytest.raises(ConfigError, match='fc_hidden_sizes'):
            dqn_specs(bad, ec)


def test_learner_and_agent_raise_before_touching_a_device():
    """the out-of-scope checks come first, so they raise on a host without a GPU"""
    import inspect
    from surreal_amd.agent import QAgentBatch
    from surreal_amd.dqn import DQNLearner
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    dp = inspect.signature(DQNLearner.__init__).parameters['dp']
    assert dp.kind is inspect.Parameter.KEYWORD_ONLY and dp.default is None
    with pytest.raises(ConfigError, match='discrete'):
        DQNLearner(lc, gym_env_config(5, 3))
    bad = copy.deepcopy(lc)
    bad.model.convs = [[16, 8, 4]]
    with pytest.raises(ConfigError, match='convs'):
        DQNLearner(bad, discrete_env_config(5, 3))
    pw = copy.deepcopy(lc)
    pw.algo.exploration.schedule = 'piecewise'
    with pytest.raises(ConfigError, match='linear'):
        QAgentBatch(pw, discrete_env_config(5, 3), 2)


def test_default_config_values():
    lc = DQN_DEFAULT_LEARNER_CONFIG
    assert lc.model.fc_hidden_sizes == [128, 128] and lc.model.dueling is True and lc.model.convs == []
    assert lc.algo.lr == 1e-3 and lc.algo.grad_norm_clipping == 10 and lc.algo.gamma == .99
    assert lc.algo.target_network_update_freq == 500 and lc.algo.double_q is True
    assert lc.algo.exploration == {'schedule': 'linear', 'steps': 10000, 'final_eps': 0.01}
    assert lc.algo.prioritized.alpha == 0.6 and lc.algo.prioritized.eps == 1e-6
    assert lc.replay.alpha == 0.6 and lc.replay.batch_size == 512
    assert lc.algo.n_step == 1 and 'parameter_publish' in lc          # BASE_LEARNER_CONFIG
    ec = discrete_env_config(7, 4)
    assert ec.action_spec == {'dim': (4,), 'type': 'discrete'}
    assert ec.obs_spec == {'low_dim': {'flat_inputs': (7,)}}


# ------------------------------------------------------------ host counter
def test_target_counter_reproduces_periodic_tracker():
    """value += 96 against period 500 over 20 steps: the copy happens when the
    value has entered the next multiple of 500 (576, 1056, 1536)"""
    mine, ref = TargetUpdateTracker(500), R.RefTracker(500)
    fired = []
    for step in range(1, 21):
        a, b = mine.track_increment(96), ref.track_increment(96)
        assert a == b and mine.value == ref.value == 96 * step and mine.endpoint == ref._endpoint
        if a:
            fired.append(step)
    assert fired == [6, 11, 16]
    with pytest.raises(ConfigError):
        TargetUpdateTracker(0)


# ------------------------------------------------------------- agent draws
def test_agent_reference_draw_order(monkeypatch):
    """q_agent.py:35-48 against a literal transcript: one random.random() per
    act (none in eval_deterministic mode), then one random.randrange(A) only
    when it did not exceed eps."""
    lc = R.dqn_config(4, [8])
    lc.algo.exploration.steps = 4
    lc.algo.exploration.final_eps = 0.5
    lc.eval.eps = 0.25
    log = []
    script = iter([0.99, 0.80, 0.60, 0.70, 0.40, 0.10, 0.30])

    def fake_random():
        v = next(script)
        log.append(('random', v))
        return v

    def fake_randrange(n):
        log.append(('randrange', n))
        return n - 1
    monkeypatch.setattr(random, 'random', fake_random)
    monkeypatch.setattr(random, 'randrange', fake_randrange)
    torch.manual_seed(3)
    agent = R.QAgentRef(lc, 2, 3, 'training')
    obs = np.array([0.5, -1.0], dtype=np.float32)
    with torch.no_grad():
        greedy = int(agent.q_func(torch.as_tensor(obs)[None]).max(1)[1])
    # eps at T = 0..4: 1.0, 0.875, 0.75, 0.625, 0.5
    acts = [agent.act(obs) for _ in range(5)]
    assert acts == [2, 2, 2, greedy, 2]
    assert log == [('random', 0.99), ('randrange', 3), ('random', 0.80), ('randrange', 3),
                   ('random', 0.60), ('randrange', 3), ('random', 0.70), ('random', 0.40),
                   ('randrange', 3)]
    assert agent.T == 5
    del log[:]
    ev = R.QAgentRef(lc, 2, 3, 'eval_stochastic')
    ev.q_func.load_state_dict(agent.q_func.state_dict())
    assert [ev.act(obs), ev.act(obs)] == [2, greedy]          # 0.10 <= 0.25 ; 0.30 > 0.25
    assert log == [('random', 0.10), ('randrange', 3), ('random', 0.30)]
    del log[:]
    det = R.QAgentRef(lc, 2, 3, 'eval_deterministic')
    det.q_func.load_state_dict(agent.q_func.state_dict())
    assert det.act(obs) == greedy and log == []
