"""model.fc_dtype = 'bf16_all' on the host (no device is touched)."""
import pytest

from surreal_amd.config import ConfigError
from surreal_amd.dqn import FC_DTYPES, FFQfunc
from tests.test_cpu_fc_dtype import _kwargs


def test_bf16_all_config():
    assert _kwargs(fc_dtype='bf16_all')[1] == {'fc_dtype': 'bf16_all'}
    assert FC_DTYPES['bf16_all'] == ('_bf16',) * 3 and FC_DTYPES['bf16'] == ('_bf16', '_bf16', '')
    with pytest.raises(ConfigError, match='noisy'):
        _kwargs(noisy=True, fc_dtype='bf16_all')
    with pytest.raises(ConfigError, match='fc_dtype'):
        FFQfunc(5, 3, [8], True, 'cpu', fc_dtype='bf16_all', noisy=0.5)


@pytest.mark.gpu
def test_clone_keeps_bf16_all():
    f = FFQfunc(5, 3, [8, 8], True, 'cuda', fc_dtype='bf16_all')
    assert f.fc_dtype == f.clone().fc_dtype == 'bf16_all'
