"""Host checks of the quantile-regression DQN configuration (surreal_amd/dqn.py)."""
import copy

import pytest

from surreal_amd.config import DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config
from surreal_amd.dqn import dqn_model_kwargs


def _kwargs(A=3, **dist):
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    lc.algo.distributional.update(dist)
    return dqn_model_kwargs(lc, discrete_env_config(5, A))


def test_quantile_keywords():
    on = _kwargs(enabled=True, kind='quantile', atoms=200, kappa=0)
    assert on[:4] == _kwargs()[:4] and on[4] == {'quantiles': 200, 'kappa': 0.0}
    assert _kwargs(enabled=True, kind='quantile', atoms=1, v_min=3, v_max=-3)[4] == {'quantiles': 1, 'kappa': 1.0}
    # categorical and disabled blocks: what they produced before the key
    assert _kwargs(kind='quantile')[4] == {} and _kwargs(kind='nonsense')[4] == {}
    assert _kwargs(enabled=True, atoms=21)[4] == {'atoms': 21, 'v_min': -10.0, 'v_max': 10.0}
    old = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    del old['algo']['distributional']['kind'], old['algo']['distributional']['kappa']
    old.algo.distributional.enabled = True
    assert dqn_model_kwargs(old, discrete_env_config(5, 3)) == _kwargs(enabled=True)


@pytest.mark.parametrize('bad', [{'kind': 'iqn'}, {'atoms': 0}, {'atoms': 257}, {'atoms': 200, 'A': 21},
                                 {'kappa': -0.5}, {'kappa': float('nan')}])
def test_quantile_ranges_raise(bad):
    with pytest.raises(ConfigError, match='distributional'):
        _kwargs(**dict({'enabled': True, 'kind': 'quantile'}, **bad))
