"""model.noisy.dtype on the host: what dqn_model_kwargs and FFQfunc accept and
refuse (no device is touched)."""
import copy

import pytest

from surreal_amd.config import DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config
from surreal_amd.dqn import FFQfunc, dqn_model_kwargs


def _kwargs(enabled=True, noisy=(), **model):
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.model.update(model)
    lc.model.noisy.update(dict(noisy), enabled=enabled)
    return dqn_model_kwargs(lc, discrete_env_config(5, 3))[4]


def test_noisy_dtype_config():
    assert 'dtype' not in DQN_DEFAULT_LEARNER_CONFIG.model.noisy
    assert _kwargs() == _kwargs(noisy={'dtype': 'fp32'}) == {'noisy': 0.5}
    for dtype in ('bf16', 'bf16_all'):
        assert _kwargs(noisy={'dtype': dtype, 'sigma0': 0.25}) == {'noisy': 0.25, 'noisy_dtype': dtype}
    for bad in ('fp16', 'BF16', None, 16):
        with pytest.raises(ConfigError, match='noisy.dtype'):
            _kwargs(noisy={'dtype': bad})
        assert _kwargs(enabled=False, noisy={'dtype': bad}) == {}        # not read when disabled
    with pytest.raises(ConfigError, match='noisy'):                      # fc_dtype is still refused
        _kwargs(fc_dtype='bf16', noisy={'dtype': 'bf16'})


def test_ffqfunc_refuses_before_it_needs_a_device():
    for kw in (dict(noisy_dtype='bf16'), dict(noisy_dtype='fp16', noisy=0.5)):
        with pytest.raises(ConfigError, match='noisy_dtype'):
            FFQfunc(5, 3, [8], True, 'cpu', **kw)
    with pytest.raises(ConfigError, match='fc_dtype'):
        FFQfunc(5, 3, [8], True, 'cpu', fc_dtype='bf16', noisy=0.5, noisy_dtype='bf16')
