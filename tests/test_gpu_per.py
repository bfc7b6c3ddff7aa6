"""Prioritized replay on the device: the tree and draw kernels against the host
mirrors (bit-equal trees, indices and MT19937 state), insert and TD updates
against tests/per_ref.py, the weighted critic loss, and PrioritizedReplay
feeding DDPGLearner (CPython-exact draws on the device's own leaves, unit
weights bit-identical to no weights, random weights on the envelope of
tests/parity.py, graph replay, pixel mode)."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch

from oracle import ddpg_ref as R
from surreal_amd import _lib as L
from surreal_amd import synthetic
from surreal_amd.config import gym_env_config, pixel_env_config
from surreal_amd.ddpg import DDPGLearner
from surreal_amd.replay import PrioritizedReplay
from tests import parity as P
from tests import per_ref as PR
from tests import test_gpu_ddpg as T
from tests.per_ref import ref_from_device
from tests.helpers import per_cfg as _per_cfg, replay_rows as _rows

pytestmark = pytest.mark.gpu


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _st():
    return L.stream(torch.device('cuda'))


def dev_tree(cap):
    tree = torch.full((int(L.lib().smi_per_tree_doubles(cap)),), float('nan'), dtype=torch.float64,
                      device='cuda')
    L.call('smi_per_init', L.ptr(tree), cap, _st())
    return tree


def dev_set(tree, cap, idx, leaves):
    i = torch.as_tensor(np.asarray(idx, dtype=np.int64), device='cuda')
    v = torch.as_tensor(np.asarray(leaves, dtype=np.float64), device='cuda')
    L.call('smi_per_set', L.ptr(tree), cap, L.ptr(i), L.ptr(v), i.numel(), _st())


def host_tree(cap, idx, leaves):
    lib = L.lib()
    tree = np.full(4 * cap, np.nan)
    assert lib.smi_per_init_host(_hp(tree), cap) == 0
    i, v = np.asarray(idx, dtype=np.int64), np.asarray(leaves, dtype=np.float64)
    assert lib.smi_per_set_host(_hp(tree), cap, _hp(i), _hp(v), len(i)) == 0
    return tree


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------------ trees
@pytest.mark.parametrize('case', PR.tree_cases(), ids=lambda c: c[0])
def test_set_device_matches_host(case):
    _, cap, idx, leaves = case
    tree = dev_tree(cap)
    dev_set(tree, cap, idx, leaves)
    assert np.array_equal(bits(tree.cpu().numpy()), bits(host_tree(cap, idx, leaves)))


def test_set_two_launches_last_occurrence_wins():
    """4096 + 5 indices on capacity 8192: the entry point launches twice; slots
    repeated inside the first launch, inside the second, and across the split
    keep their last value"""
    cap, n = 8192, 4096 + 5
    r = np.random.RandomState(9)
    idx = r.permutation(cap)[:n].astype(np.int64)
    idx[4094] = idx[10]              # repeated inside the first launch
    idx[4097] = idx[4095]            # straddles the split
    idx[4100] = idx[4096]            # inside the second launch
    idx[4099] = idx[20]              # first launch, then second
    leaves = PR.spread_leaves(n, 10)
    tree = dev_tree(cap)
    dev_set(tree, cap, idx, leaves)
    got = tree.cpu().numpy()
    assert np.array_equal(bits(got), bits(host_tree(cap, idx, leaves)))
    for k in (4094, 4097, 4100, 4099):
        assert got[2 * (cap + idx[k])] == leaves[k]


# ------------------------------------------------------------------- draw
@pytest.mark.parametrize('cap', PR.DRAW_CAPS)
@pytest.mark.parametrize('which', range(4))
def test_sample_device_matches_host(cap, which):
    lib = L.lib()
    length = PR.draw_lengths(cap)[which]
    leaves = PR.draw_tree(cap, length)
    ht = host_tree(cap, np.arange(length), leaves[:length])
    tree = torch.as_tensor(ht, device='cuda')
    ref = PR.PerRef.from_leaves(cap, leaves)
    for batch in PR.DRAW_BATCHES:
        for advanced in (False, True):
            hs = PR.seed_stream(advanced)
            assert not advanced or int(hs[624]) % 2 == 1
            hidx, hw = np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.float32)
            ds = torch.as_tensor(hs.view(np.int32).copy(), device='cuda')
            assert lib.smi_per_sample_host(_hp(ht), cap, length, _hp(hs), batch, 0.4, _hp(hidx),
                                           _hp(hw)) == 0
            idx = torch.full((batch,), -1, dtype=torch.int64, device='cuda')
            w = torch.zeros(batch, dtype=torch.float32, device='cuda')
            L.call('smi_per_sample', L.ptr(tree), cap, length, L.ptr(ds), batch, 0.4, L.ptr(idx),
                   L.ptr(w), _st())
            tag = (cap, length, batch, advanced)
            assert idx.cpu().tolist() == hidx.tolist(), tag
            assert np.array_equal(ds.cpu().numpy().view(np.uint32), hs), tag
            assert length - 1 not in hidx.tolist()
            w64 = np.asarray(ref.weights(hidx.tolist(), length, 0.4))
            assert np.all(np.abs(w.cpu().numpy().astype(np.float64) - w64) <= 2.0 ** -23 * w64), tag
    # beta = 0: exactly 1.0f
    ds = torch.as_tensor(PR.seed_stream(False).view(np.int32).copy(), device='cuda')
    idx = torch.zeros(37, dtype=torch.int64, device='cuda')
    w = torch.zeros(37, dtype=torch.float32, device='cuda')
    L.call('smi_per_sample', L.ptr(tree), cap, length, L.ptr(ds), 37, 0.0, L.ptr(idx), L.ptr(w), _st())
    assert torch.equal(w.cpu(), torch.ones(37))


# ----------------------------------------------------------------- insert
def _check_against_ref(tree, cap, ref, leaf_ulps):
    """leaves within leaf_ulps fp64 ulps of per_ref's (0: bit-equal); every
    ancestor exact given the device's own leaves; max_priority equal"""
    mine, t = ref_from_device(tree, cap)
    want = np.asarray(ref.sum[cap:])
    got = t[2 * cap::2]
    assert np.all(np.abs(got - want) <= leaf_ulps * np.spacing(want)), (got, want)
    assert np.array_equal(np.isinf(t[2 * cap + 1::2]), np.asarray(ref.min[cap:]) == np.inf)
    assert np.array_equal(bits(t), bits(mine.buffer()))
    assert t[0] == ref.max_priority


def test_insert_wraps_and_overfills():
    """memory_size 10 (capacity 16): 7 + 7 rows (wraps) at max_priority 1.0
    (1.0 ** alpha is exact: the whole tree bit-equal), then max_priority raised
    and 25 rows, more than the ring holds.  The raised leaf is a device fp64
    pow: it is held to 16 ulp, the bound OpenCL sets for a conforming fp64 pow
    (the OCML one documents less); the ancestors are exact on those leaves."""
    mem, cap, alpha = 10, 16, 0.6
    tree, ref = dev_tree(cap), PR.PerRef(cap)
    first = 0
    for n in (7, 7):
        L.call('smi_per_insert', L.ptr(tree), cap, first, n, mem, alpha, _st())
        ref.insert(first, n, mem, alpha)
        first = (first + n) % mem
        assert np.array_equal(bits(tree.cpu().numpy()), bits(ref.buffer()))
    assert np.isinf(tree.cpu().numpy()[2 * (cap + 10) + 1])          # slots past the ring stay empty
    tree[0] = 3.7
    ref.max_priority = 3.7
    L.call('smi_per_insert', L.ptr(tree), cap, first, 25, mem, alpha, _st())
    ref.insert(first, 25, mem, alpha)
    _check_against_ref(tree, cap, ref, 16)
    assert np.all(tree.cpu().numpy()[2 * cap:2 * (cap + mem):2] > 2.0)    # every ring slot rewritten


# -------------------------------------------------------------- TD update
def test_update_td_against_python():
    """64 TD errors with negatives, exact zeros and repeated indices.  Every
    leaf within alpha * 2**-24 relative of Python's (abs(float(td)) + eps) **
    alpha: less than the effect of one float32 rounding of the TD error itself
    (a float32 pow fails it); ancestors exact on the device's leaves;
    max_priority the fp64 maximum."""
    cap, n, alpha, eps = 256, 64, 0.6, 1e-6
    r = np.random.RandomState(4)
    td = (r.randn(n) * 3).astype(np.float32)
    td[[3, 17, 40]] = 0.0
    idx = r.permutation(200)[:n].astype(np.int64)
    idx[20], idx[41], idx[63] = idx[5], idx[5], idx[17]          # repeats: the last one stands
    assert (td < 0).any() and np.abs(td).max() > 1.0
    tree = dev_tree(cap)
    base_idx, base = np.arange(210), PR.spread_leaves(210, 8)
    dev_set(tree, cap, base_idx, base)
    ref = PR.PerRef(cap)
    ref.set(base_idx, base)
    di, dt = torch.as_tensor(idx, device='cuda'), torch.as_tensor(td, device='cuda')
    L.call('smi_per_update_td', L.ptr(tree), cap, L.ptr(di), L.ptr(dt), 1, n, eps, alpha, _st())
    ref.update_from_td(idx, td, eps, alpha)
    mine, t = ref_from_device(tree, cap)
    want, got = np.asarray(ref.sum[cap:]), t[2 * cap::2]
    assert np.all(np.abs(got - want) <= alpha * 2.0 ** -24 * want)
    untouched = np.setdiff1d(np.arange(cap), idx)
    assert np.array_equal(bits(got[untouched]), bits(want[untouched]))
    assert np.array_equal(bits(t[2 * cap + 1::2][idx]), bits(got[idx]))      # min leaves too
    assert np.array_equal(bits(t), bits(mine.buffer()))
    assert t[0] == max(1.0, max(abs(float(x)) + eps for x in td)) == ref.max_priority


def test_update_td_strided_column():
    """td read through its stride (a [B, 1] view of a wider matrix)"""
    cap, n = 64, 37
    wide = torch.randn(n, 3, device='cuda')
    idx = torch.randperm(cap, device='cuda')[:n]
    a, b = dev_tree(cap), dev_tree(cap)
    L.call('smi_per_update_td', L.ptr(a), cap, L.ptr(idx), L.ptr(wide[:, 1]), 3, n, 1e-6, 0.6, _st())
    col = wide[:, 1].contiguous()
    L.call('smi_per_update_td', L.ptr(b), cap, L.ptr(idx), L.ptr(col), 1, n, 1e-6, 0.6, _st())
    assert torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


# ---------------------------------------------------- weighted critic loss
@pytest.mark.parametrize('n', [1, 37, 512])
def test_mse_grad_weighted(n):
    g = torch.Generator().manual_seed(n)
    q, y = torch.randn(n, 1, generator=g), torch.randn(n, 1, generator=g)
    w = torch.rand(n, 1, generator=g) + 0.01
    qd, yd, wd = q.cuda(), y.cuda(), w.cuda()

    def run(name, wt, td):
        dq, loss = torch.full((n, 1), 9.0, device='cuda'), torch.full((1,), 9.0, device='cuda')
        if name == 'smi_mse_grad':
            L.call(name, L.ptr(qd), 1, L.ptr(yd), n, L.ptr(dq), L.ptr(loss), _st())
        else:
            L.call(name, L.ptr(qd), 1, L.ptr(yd), L.ptr(wt), n, L.ptr(dq), L.ptr(loss), L.ptr(td),
                   _st())
        return dq.cpu(), loss.cpu()
    base = run('smi_mse_grad', None, None)
    td = torch.full((n,), 9.0, device='cuda')
    for wt, t in ((None, None), (None, td), (torch.ones(n, 1, device='cuda'), td)):
        got = run('smi_mse_grad_weighted', wt, t)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    dq, loss = run('smi_mse_grad_weighted', wd, td)
    assert torch.equal(td.cpu(), (q - y).view(-1))
    q64, y64, w64 = q.double(), y.double(), w.double()
    T._fp32_as_good_as_torch(dq, (2 * (q - y) / n) * w, (2 * (q64 - y64) / n) * w64)
    T._fp32_as_good_as_torch(loss, (w * (q - y) ** 2).mean().view(1),
                             (w64 * (q64 - y64) ** 2).mean().view(1))


# ------------------------------------------------ replay + learner, end to end
def test_prioritized_replay_feeds_learner():
    B, D, A, seed = 64, 17, 6, 4321
    lc, ec = _per_cfg(B, 200), gym_env_config(D, A)
    rep = PrioritizedReplay(lc, ec, seed=seed)
    assert rep.capacity == 256 and rep.alpha == 0.6
    rows = _rows(150, D, A, 3)
    rep.insert_rows(rows)
    learner = DDPGLearner(lc, ec, seed=1)
    random.seed(seed)
    seen_max = 1.0
    for it in range(3):
        ref, t = ref_from_device(rep.tree, rep.capacity)
        if it == 0:
            assert np.array_equal(t[2 * 256:2 * (256 + 150):2], np.ones(150)) and t[0] == 1.0
        want, w64 = ref.sample(150, B, 0.4)
        idx, batch = rep.sample_batch(B, beta=0.4)
        assert idx.cpu().tolist() == want, it
        w = batch['weights']
        assert w.dtype == torch.float32 and tuple(w.shape) == (B, 1) and w.is_cuda
        w64 = np.asarray(w64)
        assert np.all(np.abs(w.cpu().numpy().reshape(-1).astype(np.float64) - w64) <= 2.0 ** -23 * w64)
        assert torch.equal(batch['obs'].cpu(), rows[want][:, :D])
        learner.learn(batch)
        td = learner.td_error
        assert tuple(td.shape) == (B,) and td.is_cuda
        assert torch.equal(td, (learner._bufs['c_q'] - learner._bufs['y']).view(-1))
        rep.update_priorities_from_td(idx, td)
        seen_max = max(seen_max, float(td.abs().max().double().item()) + 1e-6)
        assert rep.max_priority == seen_max
    assert np.array_equal(rep.rng.dev.cpu().numpy().view(np.uint32), PR.mt_state())


def test_update_priorities_host_and_device_inputs():
    lc, ec = _per_cfg(8, 10), gym_env_config(3, 2)
    rep = PrioritizedReplay(lc, ec, seed=0)
    rep.insert_rows(_rows(10, 3, 2, 0))
    ref = PR.PerRef(16)
    ref.insert(0, 10, 10, 0.6)
    idx, pr = [3, 9, 3, 0], [0.5, 2.5, 4.0, 1e-3]
    rep.update_priorities(idx, pr)
    ref.update_priorities(idx, pr, 0.6)
    assert np.array_equal(bits(rep.tree.cpu().numpy()), bits(ref.buffer()))      # host pow: bit-equal
    rep.update_priorities(torch.tensor([1, 2], device='cuda'),
                          torch.tensor([7.0, 0.25], dtype=torch.float64, device='cuda'))
    ref.update_priorities([1, 2], [7.0, 0.25], 0.6)
    _check_against_ref(rep.tree, 16, ref, 16)
    with pytest.raises(ValueError):
        rep.update_priorities([1], [0.0])


def _learner_state(learner):
    out = dict(T._ddpg_state(learner))
    for name, o in learner.opt.items():
        for k in ('m', 'v', 'step'):
            out[f'{name}.{k}'] = o[k].detach().cpu().clone()
    return out


def _assert_same(a, b, tag):
    sa, sb = _learner_state(a), _learner_state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (tag, k)
    assert a.last_stats() == b.last_stats(), tag
    assert torch.equal(a.td_error, b.td_error), tag


def test_unit_weights_change_nothing():
    B, D, A = 64, 17, 6
    lc = _per_cfg(B, double=True)
    plain = DDPGLearner(lc, gym_env_config(D, A), seed=3)
    unit = DDPGLearner(lc, gym_env_config(D, A), seed=3)
    ones = torch.ones(B, 1, device='cuda')
    for it in range(3):
        b = {k: v.cuda() for k, v in synthetic.ddpg_batch(B, D, A, seed=10 + it).items()}
        plain.learn(b)
        unit.learn(dict(b, weights=ones))
        _assert_same(plain, unit, it)


def test_graph_replay_with_weights_bit_exact():
    """the weights are one more static graph input; a graph captured with
    weights is not reused without them (steps 3, 4 capture and replay anew)"""
    B, D, A = 64, 17, 6
    lc = _per_cfg(B)
    eager = DDPGLearner(lc, gym_env_config(D, A), seed=3)
    graph = DDPGLearner(lc, gym_env_config(D, A), seed=3, use_graph=True)
    for it in range(5):
        b = {k: v.cuda() for k, v in synthetic.ddpg_batch(B, D, A, seed=10 + it).items()}
        if it < 3:
            b['weights'] = torch.rand(B, 1, generator=torch.Generator().manual_seed(it)).cuda() + 0.05
        eager.learn(b)
        graph.learn(b)
        torch.cuda.synchronize()
        _assert_same(eager, graph, it)
        assert graph._graph is not None and len(graph._gin) == (6 if it < 3 else 5)


class WeightedRef(R.DDPGLearnerRef):
    """oracle.ddpg_ref.DDPGLearnerRef with the two critic loss lines reading
    mean(w (Q - y)^2): while optimize() runs, the oracle module's `nn` is a
    stand-in whose MSELoss() is that loss (optimize uses nn.MSELoss and
    nn.utils only), so every other line is the oracle's own.  `weights` [B]
    follow the variant's row order (noise_perm) and input noise; the first
    critic's gradient is kept as it stands at its optimizer step."""
    weights = None
    weight_noise = None

    def optimize(self, obs, actions, rewards, obs_next, done):
        w = torch.as_tensor(self.weights, dtype=torch.float32).view(-1)
        if self.noise_perm is not None:
            w = w[torch.as_tensor(np.asarray(self.noise_perm).copy())]
        if self.weight_noise is not None:
            w = self.weight_noise(w)
        w = w.to(self.dtype).view(-1, 1)
        shim = types.SimpleNamespace(MSELoss=lambda: (lambda q, y: (w * (q - y) ** 2).mean()),
                                     utils=torch.nn.utils)
        step = self.critic_optim.step

        def keep_grad_then_step(*a, **k):
            self.critic_grad = R.flat_of([p.grad for p in self.critic.params()]).double().numpy().copy()
            return step(*a, **k)
        saved, R.nn, self.critic_optim.step = R.nn, shim, keep_grad_then_step
        try:
            return super().optimize(obs, actions, rewards, obs_next, done)
        finally:
            R.nn, self.critic_optim.step = saved, step


@pytest.mark.parametrize('td3', [False, True])
def test_random_weights_on_the_envelope(td3):
    """first-step critic gradient and post-step parameters against the fp64
    weighted oracle, within 2x the widest fp32 variant's distance (+ 1e-6 of
    scale): the variants ddpg_envelope_run builds (three row orders in fp32,
    six fp64 runs with one float32 rounding of input noise)"""
    B, D, A, iters = 64, 17, 6, 2
    lc = _per_cfg(B, double=td3, action_reg=td3)
    learner = DDPGLearner(lc, gym_env_config(D, A), seed=2)
    init = {k: v for k, v in T._ddpg_state(learner).items() if k in ('actor', 'critic', 'critic2')}
    batches = [{k: v.numpy() for k, v in synthetic.ddpg_batch(B, D, A, seed=it).items()}
               for it in range(iters)]
    ws = [np.random.RandomState(70 + it).uniform(0.05, 1.0, size=B).astype(np.float32)
          for it in range(iters)]
    r64 = WeightedRef(lc, D, A, dtype=torch.float64)
    T._load_ddpg(r64, init)
    vs = [T._DVariant('order', k, lc, D, A, init) for k in T.DDPG_ORDERS]
    vs += [T._DVariant('ulp', k, lc, D, A, init) for k in range(1, 7)]
    for v in vs:
        v.ref.__class__ = WeightedRef
        v.ref.weight_noise = v._noisy if v.kind == 'ulp' else None
    report = {}
    for it, b in enumerate(batches):
        np.random.seed(100 + it)
        dev = {k: torch.as_tensor(x, dtype=torch.float32).cuda() for k, x in b.items()}
        dev['weights'] = torch.as_tensor(ws[it]).cuda().view(B, 1)
        learner.learn(dev)
        got, got_grad = T._ddpg_state(learner), learner.opt['critic']['g'].detach().cpu().numpy()
        np.random.seed(100 + it)
        f64 = lambda k: torch.as_tensor(b[k], dtype=torch.float32).double()  # noqa: E731
        r64.weights = ws[it]
        r64.optimize(f64('obs'), f64('actions'), f64('rewards'), f64('obs_next'), f64('dones'))
        for v in vs:
            np.random.seed(100 + it)
            v.ref.weights = ws[it]
            v.optimize(b, it)
        if it == 0:
            wd, sc = P.width(r64.critic_grad, [v.ref.critic_grad for v in vs])
            P.check('critic_grad@0', got_grad, r64.critic_grad, wd, sc, report)
        p64 = T._ddpg_ref_state(r64)
        pvs = [T._ddpg_ref_state(v.ref) for v in vs]
        for k in p64:
            wd, sc = P.width(p64[k], [x[k] for x in pvs])
            P.check(f'{k}@{it}', got[k], p64[k], wd, sc, report)
    P.print_report(report)


# ------------------------------------------------------------------ pixel
def test_pixel_mode_gathers_the_prioritized_draw():
    D, A, cam, mem, B = 5, 2, (3, 20, 20), 16, 37
    lc = _per_cfg(B, mem)
    rep = PrioritizedReplay(lc, pixel_env_config(D, A, cam), seed=11)
    g = torch.Generator().manual_seed(1)
    rows = _rows(mem, D, A, 2)
    pix = torch.randint(0, 256, (mem,) + cam, generator=g, dtype=torch.uint8)
    pix_next = torch.randint(0, 256, (mem,) + cam, generator=g, dtype=torch.uint8)
    rep.insert_rows(rows, pix, pix_next)
    rep.update_priorities(np.arange(mem), PR.spread_leaves(mem, 3))
    ref, _ = ref_from_device(rep.tree, rep.capacity)
    random.seed(11)
    want, w64 = ref.sample(mem, B, 0.4)
    idx, batch = rep.sample_batch(B, beta=0.4)
    assert idx.cpu().tolist() == want
    assert torch.equal(batch['obs']['pixel']['camera0'].cpu(), pix[want])
    assert torch.equal(batch['obs_next']['pixel']['camera0'].cpu(), pix_next[want])
    assert torch.equal(batch['obs']['low_dim']['flat_inputs'].cpu(), rows[want][:, :D])
    assert torch.equal(batch['actions'].cpu(), rows[want][:, D:D + A])
    w = batch['weights']
    assert w.dtype == torch.float32 and tuple(w.shape) == (B, 1)
    w64 = np.asarray(w64)
    assert np.all(np.abs(w.cpu().numpy().reshape(-1).astype(np.float64) - w64) <= 2.0 ** -23 * w64)
    with pytest.raises(ValueError):
        rep.sample(B)                               # pixel replays sample through sample_batch


def test_world_2_raises():
    rep = PrioritizedReplay(_per_cfg(8, 16), gym_env_config(3, 2), seed=0)
    rep.insert_rows(_rows(12, 3, 2, 0))
    with pytest.raises(ValueError):
        rep.sample_batch(8, rank=0, world=2)
    with pytest.raises(ValueError):
        rep.sample(8, rank=1, world=2)
    idx, rows, w = rep.sample(8, beta=0.5)
    assert tuple(rows.shape) == (8, rep.width) and tuple(w.shape) == (8,)
