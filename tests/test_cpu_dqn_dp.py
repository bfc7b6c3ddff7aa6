"""Data-parallel DQN, host side (no GPU): the argument checks of
smi_dqn_td_shard, which return before any launch, and the decomposition the
shard kernel and DQNLearner(dp=...) implement, on the fp64 reference: the sum
over equal shards of the gradients of sum(w * huber) / B_global is the gradient
of mean(w * huber) over the global batch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dqn_ref as R

E_ARG = -1


def test_shard_entry_rejects_bad_arguments_before_any_launch():
    from surreal_amd import _lib
    assert 'smi_dqn_td_shard' in _lib.exported_symbols()
    lib = _lib.lib()
    host = (ctypes.c_float * 64)()              # never read: every call below fails validation
    p = ctypes.cast(host, ctypes.c_void_p)
    ok = dict(adv=p, lda=3, adv_n=p, ldn=3, adv_t=p, ldt=3, val=p, vs=1, val_n=p, vns=1, val_t=p,
              vts=1, act=p, as_=1, rew=p, rs=1, done=p, ds=1, w=None, B=4, Bg=8, row0=4, A=3,
              gamma=0.99, dueling=1, double_q=1, dadv=p, ldd=3, dval=p, td=p, y=None, stats=p)
    bad = [(dict(row0=5), 'row0 + B > B_global'), (dict(Bg=3, row0=0), 'B_global < B'),
           (dict(row0=-1), 'row0 < 0'), (dict(row0=2 ** 62), 'row0 + B > B_global'),
           (dict(adv=None), 'null'), (dict(adv_t=None), 'null'), (dict(act=None), 'null'),
           (dict(rew=None), 'null'), (dict(done=None), 'null'), (dict(dadv=None), 'null'),
           (dict(td=None), 'null'), (dict(stats=None), 'null'), (dict(adv_n=None), 'null'),
           (dict(val=None), 'dueling'), (dict(dval=None), 'dueling'), (dict(B=0), 'B < 1'),
           (dict(A=0), 'A < 1'), (dict(ldd=2), 'leading')]
    for kw, word in bad:
        a = dict(ok, **kw)
        rc = lib.smi_dqn_td_shard(*a.values(), None)
        msg = lib.smi_last_error().decode()
        assert rc == E_ARG, (kw, rc)
        assert 'dqn_td_shard' in msg and word in msg, (kw, msg)
    with pytest.raises(RuntimeError):
        _lib.check(E_ARG, 'smi_dqn_td_shard')


def test_dp_is_a_keyword_and_host_checks_still_come_first():
    """DQNLearner(dp=...) is accepted as a keyword; the out-of-scope checks raise
    before the group or a device is looked at; any other keyword is a TypeError"""
    import copy
    from surreal_amd.config import (DQN_DEFAULT_LEARNER_CONFIG, ConfigError, discrete_env_config,
                                    gym_env_config)
    from surreal_amd.dqn import DQNLearner
    lc = copy.deepcopy(DQN_DEFAULT_LEARNER_CONFIG)
    with pytest.raises(ConfigError, match='discrete'):
        DQNLearner(lc, gym_env_config(5, 3), dp=object())
    with pytest.raises(ConfigError, match='discrete'):
        DQNLearner(lc, gym_env_config(5, 3), dp=None)
    with pytest.raises(TypeError, match='world'):
        DQNLearner(lc, discrete_env_config(5, 3), world=2)


def _grad(ref):
    return np.concatenate([p.grad.double().numpy().reshape(-1) for p in ref.q_func.parameters()])


@pytest.mark.parametrize('world', [2, 3, 4])
def test_shard_gradients_sum_to_the_global_gradient(world):
    lc, D, A, init, batches = R.envelope_case('b96_duel_dq')
    b = batches[0]
    assert 'weights' in b
    B = b['obs'].shape[0]
    n = B // world
    assert n * world == B
    ref = R.DQNLearnerRef(lc, D, A, torch.float64)
    ref.load(init)
    f64 = lambda k, lo=0, hi=B: torch.as_tensor(b[k][lo:hi], dtype=torch.float32).double()  # noqa: E731
    _, td = ref.optimize(f64('obs'), b['actions'], f64('rewards'), f64('obs_next'), f64('dones'),
                         f64('weights'), step=False)
    g_global = _grad(ref)
    g_sum, tds = np.zeros_like(g_global), []
    for r in range(world):
        lo, hi = r * n, (r + 1) * n
        # the reference's loss on the shard is mean over n rows: times n / B it is
        # sum(w * huber) / B_global, and so is its gradient
        _, td_r = ref.optimize(f64('obs', lo, hi), b['actions'][lo:hi], f64('rewards', lo, hi),
                               f64('obs_next', lo, hi), f64('dones', lo, hi),
                               f64('weights', lo, hi), step=False)
        g_sum += _grad(ref) * (n / B)
        tds.append(td_r.numpy())
    assert np.abs(g_global).max() > 0
    rel = np.abs(g_sum - g_global).max() / np.abs(g_global).max()
    print('shard gradient sum against the global gradient, relative:', rel)
    assert rel <= 1e-12
    # rows do not see their shard (the GEMM blocking may differ with the row count)
    assert np.allclose(np.concatenate(tds), td.numpy(), rtol=1e-12, atol=1e-12)
