"""model.conv_dtype on the host: what dqn_model_kwargs accepts and refuses (no
device is touched)."""
import copy

import pytest

from surreal_amd.config import (DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config,
                                discrete_pixel_env_config)
from surreal_amd.dqn import dqn_model_kwargs


def _kwargs(pixel=True, **model):
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.model.convs = [[8, 8, 4], [16, 3, 1]] if pixel else []
    lc.model.update(model)
    ec = discrete_pixel_env_config((4, 20, 20), 3) if pixel else discrete_env_config(5, 3)
    return lc, dqn_model_kwargs(lc, ec)[4]


def test_conv_dtype_config():
    lc, default = _kwargs()
    assert 'conv_dtype' not in default and lc.model.conv_dtype == 'fp32'
    del lc['model']['conv_dtype']                                    # a config from before the key
    assert dqn_model_kwargs(lc, discrete_pixel_env_config((4, 20, 20), 3))[4] == default
    assert _kwargs(conv_dtype='fp32')[1] == default
    assert _kwargs(conv_dtype='bf16')[1] == dict(default, conv_dtype='bf16')
    assert _kwargs(pixel=False, conv_dtype='fp32')[1] == {}
    for bad in ('fp16', 'BF16', None, 16):
        with pytest.raises(ConfigError, match='conv_dtype'):
            _kwargs(conv_dtype=bad)
    with pytest.raises(ConfigError, match='convs'):
        _kwargs(pixel=False, conv_dtype='bf16')
