"""Data-parallel DDPG with a prioritized replay, host side (no GPU): the
argument checks of smi_mse_grad_weighted_shard, which return before any launch,
and the decomposition DDPGLearner(dp=...) relies on, on the fp64 weighted
oracle: the mean over equal shards of the shard's critic gradient of
mean(w (Q - y)^2) is the global batch's gradient (the shard kernel divides by
its own row count; the exchange averages)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ddpg_ref as R
from surreal_amd import synthetic
from tests.helpers import per_cfg as _per_cfg
from tests.test_gpu_ddpg import _load_ddpg
from tests.test_gpu_per import WeightedRef

E_ARG = -1


def test_shard_entry_rejects_bad_arguments_before_any_launch():
    from surreal_amd import _lib
    assert 'smi_mse_grad_weighted_shard' in _lib.exported_symbols()
    lib = _lib.lib()
    host = (ctypes.c_float * 64)()              # never read: every call below fails validation
    p = ctypes.cast(host, ctypes.c_void_p)
    ok = dict(q=p, qs=1, y=p, w=None, n=4, ng=8, row0=4, dq=p, loss=None, td=p)
    bad = [(dict(q=None), 'null'), (dict(y=None), 'null'), (dict(dq=None), 'null'),
           (dict(td=None), 'null'), (dict(n=0), 'n < 1'), (dict(n=-3), 'n < 1'),
           (dict(ng=3, row0=0), 'n_global < n'), (dict(row0=-1), 'row0 < 0'),
           (dict(row0=5), 'row0 + n > n_global'), (dict(row0=2 ** 62), 'row0 + n > n_global'),
           (dict(row0=2 ** 63 - 1), 'row0 + n > n_global')]
    for kw, word in bad:
        a = dict(ok, **kw)
        rc = lib.smi_mse_grad_weighted_shard(*a.values(), None)
        msg = lib.smi_last_error().decode()
        assert rc == E_ARG, (kw, rc)
        assert 'mse_grad_weighted_shard' in msg and word in msg, (kw, msg)
    with pytest.raises(RuntimeError):
        _lib.check(E_ARG, 'smi_mse_grad_weighted_shard')


B, D, A = 96, 17, 6


def _critic_grads(lc, init, b, w, lo, hi):
    """fp64 gradients of the critic(s) of a fresh weighted oracle on rows [lo, hi)"""
    ref = WeightedRef(lc, D, A, dtype=torch.float64)
    ref.batch_size = hi - lo
    _load_ddpg(ref, init)
    ref.weights = w[lo:hi]
    f64 = lambda k: torch.as_tensor(b[k][lo:hi], dtype=torch.float32).double()  # noqa: E731
    ref.optimize(f64('obs'), f64('actions'), f64('rewards'), f64('obs_next'), f64('dones'))
    g = [ref.critic_grad]
    if ref.double:      # the twin's gradient is still on its parameters after its step
        g.append(R.flat_of([p.grad for p in ref.critic2.params()]).double().numpy().copy())
    return np.concatenate(g)


@pytest.mark.parametrize('world', [2, 3, 4])
@pytest.mark.parametrize('twin', [False, True], ids=['plain', 'twin'])
def test_mean_of_shard_gradients_is_the_global_gradient(twin, world):
    lc = _per_cfg(B, double=twin)
    src = R.DDPGLearnerRef(lc, D, A, seed=3, dtype=torch.float64)
    init = {'actor': R.flat_of(src.actor.params()), 'critic': R.flat_of(src.critic.params())}
    if twin:
        init['critic2'] = R.flat_of(src.critic2.params())
    b = {k: v.numpy() for k, v in synthetic.ddpg_batch(B, D, A, seed=0).items()}
    w = np.random.RandomState(70).uniform(0.05, 1.0, size=B).astype(np.float32)
    n = B // world
    assert n * world == B
    g_global = _critic_grads(lc, init, b, w, 0, B)
    g_mean = sum(_critic_grads(lc, init, b, w, r * n, (r + 1) * n) for r in range(world)) / world
    assert np.abs(g_global).max() > 0
    rel = np.abs(g_mean - g_global).max() / np.abs(g_global).max()
    print('mean of the shard gradients against the global gradient, relative:', rel)
    assert rel <= 1e-12
