"""Host checks of the categorical (C51) DQN configuration (surreal_amd/dqn.py)."""
import copy

import pytest

from surreal_amd.config import DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config
from surreal_amd.dqn import dqn_model_kwargs


def _kwargs(**dist):
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.algo.distributional.update(dist)
    return dqn_model_kwargs(lc, discrete_env_config(5, 3))


def test_distributional_keywords():
    assert _kwargs()[4] == {} and _kwargs(atoms=1)[4] == {}          # disabled: nothing is read
    old = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    del old['algo']['distributional']                                # a config from before the block
    assert dqn_model_kwargs(old, discrete_env_config(5, 3)) == _kwargs()
    on = _kwargs(enabled=True, atoms=21, v_max=5)
    assert on[:4] == _kwargs()[:4] and on[4] == {'atoms': 21, 'v_min': -10.0, 'v_max': 5.0}


@pytest.mark.parametrize('bad', [{'atoms': 1}, {'atoms': 65}, {'v_max': -10.0}, {'v_min': 11.0}])
def test_distributional_ranges_raise(bad):
    with pytest.raises(ConfigError, match='distributional'):
        _kwargs(enabled=True, **bad)
