"""Implicit quantile DQN on the host: the range checks, the flat layout and what
the other kinds' configurations still produce."""
import pytest

from surreal_amd.config import ConfigError, discrete_env_config
from surreal_amd.dqn import check_implicit, dqn_model_kwargs
from tests import dqn_ref as R


def _kwargs(**dist):
    lc = R.dqn_config(32, [16], True, True)
    lc.algo.distributional.update(enabled=True, **dist)
    return dqn_model_kwargs(lc, discrete_env_config(5, 6))[4]


@pytest.mark.parametrize('ok,bad', [
    (dict(atoms=1), dict(atoms=0)), (dict(atoms=64), dict(atoms=65)),
    (dict(target_atoms=1), dict(target_atoms=0)), (dict(target_atoms=64), dict(target_atoms=65)),
    (dict(act_atoms=1), dict(act_atoms=0)), (dict(act_atoms=64), dict(act_atoms=65)),
    (dict(embed_dim=4), dict(embed_dim=0)), (dict(embed_dim=64), dict(embed_dim=68)),
    (dict(embed_dim=8), dict(embed_dim=6)), (dict(kappa=0.0), dict(kappa=-0.5))])
def test_implicit_range_edges(ok, bad):
    assert _kwargs(kind='implicit', **ok)['implicit'] == check_implicit(6, **{'atoms': 51, **ok})
    with pytest.raises(ConfigError):
        _kwargs(kind='implicit', **bad)


def test_implicit_slab_edge_and_defaults():
    assert check_implicit(64, 8, None, 64) == {'atoms': 8, 'target_atoms': 8, 'act_atoms': 64,
                                               'embed_dim': 64, 'kappa': 1.0}
    assert check_implicit(6)['act_atoms'] == 32 and check_implicit(6)['atoms'] == 8
    for kw in (dict(atoms=64), dict(target_atoms=64), dict(act_atoms=64)):
        with pytest.raises(ConfigError):
            check_implicit(65, **{'atoms': 8, 'act_atoms': 8, **kw})


def test_other_kinds_produce_what_they_did():
    assert _kwargs(kind='categorical', atoms=51) == {'atoms': 51, 'v_min': -10.0, 'v_max': 10.0}
    assert _kwargs(kind='quantile', atoms=200, kappa=0.5) == {'quantiles': 200, 'kappa': 0.5}
    lc = R.dqn_config(32, [16], True, True)
    assert dqn_model_kwargs(lc, discrete_env_config(5, 6))[4] == {}
    with pytest.raises(ConfigError):
        _kwargs(kind='mixture')


@pytest.mark.gpu
@pytest.mark.parametrize('dueling,hidden', [(True, [16, 8]), (False, [12])])
def test_implicit_layout_appends_to_the_scalar_one(dueling, hidden):
    """every pre-existing offset is the scalar model's (by formula); fc_tau_layer follows"""
    from surreal_amd.dqn import FFQfunc
    D, A, S, n_cos = 5, 3, 2 if dueling else 1, 12
    f = FFQfunc(D, A, hidden, dueling, 'cuda', implicit={'embed_dim': n_cos})
    offs = {k: f.off(v) for k, v in f.named_parameters()}
    widths = hidden + [A]
    deep = lambda out: sum(o * i + o for i, o in zip(hidden, hidden[1:] + [out]))      # noqa: E731
    n = S * hidden[0] * (D + 1) + deep(A) + (deep(1) if dueling else 0)
    assert offs['fc_action_layers.0.weight'] == 0 and offs['fc_action_layers.0.bias'] == S * hidden[0] * D
    assert offs['fc_action_layers.1.weight'] == S * hidden[0] * (D + 1)
    if dueling:
        assert offs['fc_state_layers.0.weight'] == hidden[0] * D
        assert offs['fc_state_layers.1.weight'] == S * hidden[0] * (D + 1) + deep(A)
    assert offs['fc_tau_layer.weight'] == n and offs['fc_tau_layer.bias'] == n + S * hidden[0] * n_cos
    assert f.flat.numel() == n + S * hidden[0] * (n_cos + 1) and len(widths) == len(hidden) + 1
    assert list(f.state_dict())[-2:] == ['fc_tau_layer.weight', 'fc_tau_layer.bias']
    assert f.clone().implicit == f.implicit
