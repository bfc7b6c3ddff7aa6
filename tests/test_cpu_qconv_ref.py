"""Pixel DQN, host side (no GPU): the power of the conv-layer checker the GPU
tests rely on (tests/qconv_ref.py), spec parsing of the conv model, and the
arg-max margin of the pixel learner cases."""
import copy

import numpy as np
import pytest
import torch

from surreal_amd.config import (DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config,
                                discrete_pixel_env_config, pixel_env_config)
from tests import qconv_ref as Q


# ------------------------------------------------------ the layer checker
@pytest.mark.parametrize('name', sorted(Q.GEOMS))
def test_checker_passes_a_correct_fp32_layer(name):
    for n in Q.NS:
        for div in ((False, True) if Q.GEOMS[name][5] else (False,)):
            Q.check_layer(Q.TorchLayer(), Q.LayerCase(name, n), div)


@pytest.mark.parametrize('fault', sorted(Q.FAULTY))
def test_checker_fails_a_faulty_layer(fault):
    impl, (name, n, div) = Q.FAULTY[fault]
    with pytest.raises(AssertionError):
        Q.check_layer(impl, Q.LayerCase(name, n), div)


def test_faults_cover_the_list():
    assert sorted(Q.FAULTY) == sorted([
        'pad_one_side', 'tf_same', 'pad_k_minus_1', 'swap_hw', 'stride_one_axis', 'no_div255',
        'ge_mask', 'dw_drops_last_image', 'no_db'])


# ------------------------------------------------------------ spec parsing
def _atari():
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.model.convs = [list(c) for c in Q.NATURE]
    lc.model.fc_hidden_sizes = [512]
    return lc, discrete_pixel_env_config((1, 84, 84), 6, frame_stacks=4)


def test_atari_config_parses():
    from surreal_amd.dqn import conv_chain, dqn_conv_specs
    lc, ec = _atari()
    assert ec.obs_spec == {'pixel': {'camera0': (4, 84, 84)}} and ec.frame_stacks == 4
    assert ec.action_spec == {'dim': (6,), 'type': 'discrete'}
    shape, convs, A, hidden, dueling, is_uint8 = dqn_conv_specs(lc, ec)
    assert (shape, A, hidden, dueling) == ((4, 84, 84), 6, [512], True)
    assert is_uint8 is True                                  # the documented default
    layers, pre = conv_chain(shape, convs)
    assert [(l[1], l[2]) for l in layers] == [(84, 84), (22, 22), (12, 12)]
    assert pre == (64, 12, 12) and int(np.prod(pre)) == 9216
    assert [l[6] for l in layers] == [4, 2, 1]               # SAME: pad = k // 2
    assert Q.conv_shapes(shape, convs) == (layers, pre)
    lc.model.is_uint8 = False
    assert dqn_conv_specs(lc, ec)[5] is False


def test_state_dict_key_order():
    """the reference's construction order (q_net.py:87-110), from the host-side
    name list the model builds its views from"""
    from surreal_amd.dqn import ffq_param_names
    names = ffq_param_names(n_convs=3, n_hidden=1, dueling=True)
    ref = Q.QConvRef((4, 84, 84), 6, Q.NATURE, [8], True, True)
    assert names == list(ref.state_dict().keys())
    ref = Q.QConvRef((2, 9, 11), 3, [[6, 3, 2]], [16, 8], False, False)
    assert ffq_param_names(1, 2, False) == list(ref.state_dict().keys())
    assert ffq_param_names(0, 2, True)[0] == 'fc_action_layers.0.weight'


def test_conv_spec_errors_raise_before_a_device_is_touched():
    from surreal_amd.agent import QAgentBatch
    from surreal_amd.dqn import DQNLearner, FFQfunc, dqn_conv_specs, dqn_specs
    lc, ec = _atari()
    low = discrete_env_config(5, 3)
    with pytest.raises(ConfigError, match='convs'):          # convs on a low-dim spec
        dqn_specs(lc, low)
    with pytest.raises(ConfigError, match='convs'):
        DQNLearner(lc, low)
    empty = copy.deepcopy(lc)
    empty.model.convs = []
    for ctor in (lambda: dqn_conv_specs(empty, ec), lambda: DQNLearner(empty, ec),
                 lambda: QAgentBatch(empty, ec, 2)):
        with pytest.raises(ConfigError, match='pixel'):      # pixels without convs
            ctor()
    both = pixel_env_config(5, 3)
    both.action_spec = {'dim': (3,), 'type': 'discrete'}
    for ctor in (lambda: dqn_conv_specs(lc, both), lambda: DQNLearner(lc, both)):
        with pytest.raises(ConfigError, match='pixel'):      # FFQfunc has one input
            ctor()
    cont = discrete_pixel_env_config((4, 84, 84), 6)
    cont.action_spec = {'dim': (6,), 'type': 'continuous'}
    with pytest.raises(ConfigError, match='discrete'):
        DQNLearner(lc, cont)
    for convs, what in (([[32, 9, 4]], 'convs'), ([[32, 8, 5]], 'convs'), ([[32, 3, 4]], 'convs'),
                        ([[129, 3, 1]], 'convs'), ([[32, 8]], 'convs'),
                        ([[8, 3, 1]] * 5, 'convs')):
        bad = copy.deepcopy(lc)
        bad.model.convs = convs
        with pytest.raises(ConfigError, match=what):
            DQNLearner(bad, ec)
        with pytest.raises(ConfigError, match=what):
            QAgentBatch(bad, ec, 2)
    big = discrete_pixel_env_config((129, 8, 8), 6)
    with pytest.raises(ConfigError, match='channels'):
        DQNLearner(lc, big)
    # an invalid pre-FC shape is the reference's ValueError (q_net.py:104-105)
    with pytest.raises(ValueError, match='Pre-FC shape'):
        FFQfunc(0, 3, [8], True, convs=[[4, 3, 1]], input_shape=(2, 0, 5))
    with pytest.raises(ValueError, match='input_shape'):
        FFQfunc(0, 3, [8], True, convs=[[4, 3, 1]], input_shape=(5,))


# ------------------------------------------------------- learner conditions
def _fp64_steps(name):
    lc, shape, A, init, batches = Q.pix_case(name)
    ref = Q.PixLearnerRef(lc, shape, A, torch.float64)
    ref.load(init)
    out = []
    for b in batches:
        ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'], b.get('weights'))
        out.append(ref.last['scanned'].numpy())
    return out


@pytest.mark.parametrize('name', sorted(Q.PIX_CASES))
def test_argmax_margin_on_every_row(name):
    """tests/test_cpu_dqn.py::test_argmax_margin_on_every_row for the pixel cases"""
    for it, scanned in enumerate(_fp64_steps(name)):
        top = np.sort(scanned, axis=1)
        gap = top[:, -1] - top[:, -2]
        assert gap.min() >= 1e-5 * np.abs(scanned).max(), (name, it, gap.min())


def test_fp32_reference_passes_the_pixel_envelope():
    lc, shape, A, init, batches = Q.pix_case('pix_plain')
    got = Q.run_pix_reference(lc, shape, A, init, batches)
    report = Q.envelope_check_pixels(lc, shape, A, init, batches, got)
    assert '_fail' not in report, report['_fail']
    bad = Q.run_pix_reference(lc, shape, A, init, batches, fault='no_dones')
    assert 'td_error@0' in Q.envelope_check_pixels(lc, shape, A, init, batches, bad).get('_fail', [])
