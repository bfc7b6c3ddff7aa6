"""model.fc_dtype on the host: what dqn_model_kwargs and FFQfunc accept and
refuse (no device is touched)."""
import copy

import pytest

from surreal_amd.config import DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config
from surreal_amd.dqn import FFQfunc, dqn_model_kwargs


def _kwargs(noisy=False, **model):
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.model.update(model)
    lc.model.noisy.enabled = noisy
    return lc, dqn_model_kwargs(lc, discrete_env_config(5, 3))[4]


def test_fc_dtype_config():
    lc, default = _kwargs()
    assert default == {} and lc.model.fc_dtype == 'fp32'
    del lc['model']['fc_dtype']                                      # a config from before the key
    assert dqn_model_kwargs(lc, discrete_env_config(5, 3))[4] == {}
    assert _kwargs(fc_dtype='fp32')[1] == {}
    assert _kwargs(fc_dtype='bf16')[1] == {'fc_dtype': 'bf16'}
    assert 'fc_dtype' not in _kwargs(noisy=True)[1]
    for bad in ('fp16', 'BF16', None, 16):
        with pytest.raises(ConfigError, match='fc_dtype'):
            _kwargs(fc_dtype=bad)
    with pytest.raises(ConfigError, match='noisy'):
        _kwargs(noisy=True, fc_dtype='bf16')


def test_ffqfunc_refuses_before_it_needs_a_device():
    for kw in (dict(fc_dtype='fp16'), dict(fc_dtype='bf16', noisy=0.5)):
        with pytest.raises(ConfigError, match='fc_dtype'):
            FFQfunc(5, 3, [8], True, 'cpu', **kw)


@pytest.mark.gpu
def test_clone_keeps_fc_dtype():
    f = FFQfunc(5, 3, [8, 8], True, 'cuda', fc_dtype='bf16')
    assert f.fc_dtype == f.clone().fc_dtype == 'bf16'
    assert FFQfunc(5, 3, [8], False, 'cuda').clone().fc_dtype == 'fp32'
