"""Noisy linear layers on the host: config parsing, the appended names and the
sigma shift, and the argument checks of the C ABI (no device is touched)."""
import copy

import pytest

from surreal_amd import _lib as L
from surreal_amd.config import DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config
from surreal_amd.dqn import (dqn_model_kwargs, ffq_noisy_layers, ffq_param_names, ffq_sigma_names,
                             ffq_sigma_shift)


def _kwargs(**noisy):
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.model.noisy.update(noisy)
    return dqn_model_kwargs(lc, discrete_env_config(5, 3))[4]


def test_noisy_config():
    old = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    del old['model']['noisy']                                        # a config from before the key
    assert dqn_model_kwargs(old, discrete_env_config(5, 3))[4] == {} == _kwargs()
    assert _kwargs(enabled=True) == {'noisy': 0.5} and _kwargs(enabled=True, sigma0=0.1) == {'noisy': 0.1}
    assert _kwargs(enabled=False, sigma0=-1) == {}
    for bad in (0, -0.5, float('inf'), float('nan'), 'x'):
        with pytest.raises(ConfigError):
            _kwargs(enabled=True, sigma0=bad)


def test_noisy_names_shift_and_layers():
    names = ffq_sigma_names(2, True)
    assert names == [n + '_sigma' for n in ffq_param_names(0, 2, True)] and len(names) == 12
    assert ffq_sigma_names(1, False) == ['fc_action_layers.0.weight_sigma', 'fc_action_layers.0.bias_sigma',
                                         'fc_action_layers.1.weight_sigma', 'fc_action_layers.1.bias_sigma']
    # [convs 100 | FC 100..1100 | tau 40 | sigma]: offset 100 -> 1140
    assert ffq_sigma_shift(100, 1100, 40) + 100 == 1140 and ffq_sigma_shift(0, 7, 0) == 7
    assert ffq_noisy_layers(5, [16, 12], True, (3, 1)) == [(5, 32), (16, 12), (12, 3), (16, 12), (12, 1)]
    assert ffq_noisy_layers(5, [16], False, (3,)) == [(5, 16), (16, 3)]


X = 64        # a non-NULL address that no check dereferences


@pytest.mark.parametrize('name,args,word', [
    ('smi_noisy_forward', [X, 4, 1, 4, X, X, 4, None, None, X, None, 4, 0, X, 4, None], 'null'),
    ('smi_noisy_forward', [X, 4, 1, 4, X, X, 4, None, None, X, X, 4, 3, X, 4, None], 'act'),
    ('smi_noisy_backward_input', [X, 4, 1, 4, X, None, 4, 4, X, X, None, 0, X, 4, None], 'null'),
    ('smi_noisy_backward_input', [X, 4, 1, 4, X, X, 4, 4, X, X, X, 3, X, 4, None], 'leading'),
    ('smi_noisy_draw', [1, None, 0, 1, L.noisy_dims([(4, 4)])[1], X, None, None], 'null'),
    ('smi_noisy_draw', [1, X, 0, 2, L.noisy_dims([(4, 4)])[1], X, None, None], 'width'),
    ('smi_noisy_sigma_grad', [X, X, X, 1, L.noisy_table([(-4, 16, 4, 4)])[1], None], 'offset'),
])
def test_noisy_calls_reject_bad_arguments(name, args, word):
    lib = L.lib()
    assert getattr(lib, name)(*args) == -1 and word in lib.smi_last_error().decode()
