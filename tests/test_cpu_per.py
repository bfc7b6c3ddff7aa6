"""Prioritized replay, host side (no GPU): argument checks of the smi_per_*
entry points, the host tree mirror against tests/per_ref.py bit for bit, and
the host draw against the live CPython generator (indices and the whole
MT19937 state bit-equal, weights within one float32 rounding of the fp64
formula)."""
import ctypes
import random

import numpy as np
import pytest

from tests import per_ref as PR


def _lib():
    from surreal_amd import _lib
    return _lib.lib()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _err(lib, rc, word):
    assert rc == -1, rc
    msg = lib.smi_last_error()
    assert word in msg, msg


def test_tree_doubles():
    lib = _lib()
    assert lib.smi_per_tree_doubles(8) == 32
    assert lib.smi_per_tree_doubles(1 << 19) == 4 << 19


def test_argument_errors():
    lib = _lib()
    cap = 8
    tree = np.zeros(4 * cap)
    idx = np.zeros(4, dtype=np.int64)
    leaf = np.ones(4)
    td = np.ones(4, dtype=np.float32)
    st = np.zeros(625, dtype=np.uint32)
    out, w = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.float32)
    T, I, Lf, D, S, O, W = (_p(a) for a in (tree, idx, leaf, td, st, out, w))
    # a capacity that is not a power of two
    for bad in (0, 6, -8):
        _err(lib, lib.smi_per_init(T, bad, None), b'power of two')
        _err(lib, lib.smi_per_init_host(T, bad), b'power of two')
        _err(lib, lib.smi_per_set(T, bad, I, Lf, 4, None), b'power of two')
        _err(lib, lib.smi_per_set_host(T, bad, I, Lf, 4), b'power of two')
        _err(lib, lib.smi_per_insert(T, bad, 0, 4, 5, 0.6, None), b'power of two')
        _err(lib, lib.smi_per_update_td(T, bad, I, D, 1, 4, 1e-6, 0.6, None), b'power of two')
        _err(lib, lib.smi_per_sample(T, bad, 4, S, 4, 0.4, O, W, None), b'power of two')
        _err(lib, lib.smi_per_sample_host(T, bad, 4, S, 4, 0.4, O, W), b'power of two')
    # len < 2, len > capacity
    for bad in (1, 0, -3, cap + 1):
        _err(lib, lib.smi_per_sample(T, cap, bad, S, 4, 0.4, O, W, None), b'len')
        _err(lib, lib.smi_per_sample_host(T, cap, bad, S, 4, 0.4, O, W), b'len')
    # eps <= 0, alpha <= 0, beta < 0
    for bad in (0.0, -1e-6):
        _err(lib, lib.smi_per_update_td(T, cap, I, D, 1, 4, bad, 0.6, None), b'eps')
        _err(lib, lib.smi_per_update_td(T, cap, I, D, 1, 4, 1e-6, bad, None), b'alpha')
        _err(lib, lib.smi_per_insert(T, cap, 0, 4, 5, bad, None), b'alpha')
    _err(lib, lib.smi_per_sample(T, cap, 4, S, 4, -0.1, O, W, None), b'beta')
    _err(lib, lib.smi_per_sample_host(T, cap, 4, S, 4, -0.1, O, W), b'beta')
    # NULL pointers
    _err(lib, lib.smi_per_init(None, cap, None), b'null')
    _err(lib, lib.smi_per_init_host(None, cap), b'null')
    for a in ((None, cap, I, Lf, 4), (T, cap, None, Lf, 4), (T, cap, I, None, 4)):
        _err(lib, lib.smi_per_set(*a, None), b'null')
        _err(lib, lib.smi_per_set_host(*a), b'null')
    _err(lib, lib.smi_per_insert(None, cap, 0, 4, 5, 0.6, None), b'null')
    for a in ((None, cap, I, D), (T, cap, None, D), (T, cap, I, None)):
        _err(lib, lib.smi_per_update_td(*a, 1, 4, 1e-6, 0.6, None), b'null')
    for a in ((None, S, O, W), (T, None, O, W), (T, S, None, W), (T, S, O, None)):
        _err(lib, lib.smi_per_sample(a[0], cap, 4, a[1], 4, 0.4, a[2], a[3], None), b'null')
        _err(lib, lib.smi_per_sample_host(a[0], cap, 4, a[1], 4, 0.4, a[2], a[3]), b'null')
    # negative counts
    _err(lib, lib.smi_per_set(T, cap, I, Lf, -1, None), b'n < 0')
    _err(lib, lib.smi_per_set_host(T, cap, I, Lf, -1), b'n < 0')
    _err(lib, lib.smi_per_insert(T, cap, 0, -1, 5, 0.6, None), b'n < 0')
    _err(lib, lib.smi_per_update_td(T, cap, I, D, 1, -1, 1e-6, 0.6, None), b'n < 0')
    _err(lib, lib.smi_per_sample(T, cap, 4, S, -1, 0.4, O, W, None), b'batch < 0')
    _err(lib, lib.smi_per_sample_host(T, cap, 4, S, -1, 0.4, O, W), b'batch < 0')
    # an insert's ring must fit the tree
    _err(lib, lib.smi_per_insert(T, cap, 0, 4, cap + 1, 0.6, None), b'memory_size')
    _err(lib, lib.smi_per_insert(T, cap, 5, 4, 5, 0.6, None), b'first_slot')


def test_zero_size_calls_return_ok_without_a_launch():
    lib = _lib()
    cap = 8
    tree = np.zeros(4 * cap)
    assert lib.smi_per_init_host(_p(tree), cap) == 0
    before = tree.copy()
    idx, leaf = np.zeros(1, dtype=np.int64), np.ones(1)
    td, st = np.ones(1, dtype=np.float32), np.zeros(625, dtype=np.uint32)
    out, w = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.float32)
    assert lib.smi_per_set(_p(tree), cap, _p(idx), _p(leaf), 0, None) == 0
    assert lib.smi_per_set_host(_p(tree), cap, _p(idx), _p(leaf), 0) == 0
    assert lib.smi_per_insert(_p(tree), cap, 0, 0, 5, 0.6, None) == 0
    assert lib.smi_per_update_td(_p(tree), cap, _p(idx), _p(td), 1, 0, 1e-6, 0.6, None) == 0
    assert lib.smi_per_sample(_p(tree), cap, 4, _p(st), 0, 0.4, _p(out), _p(w), None) == 0
    assert lib.smi_per_sample_host(_p(tree), cap, 4, _p(st), 0, 0.4, _p(out), _p(w)) == 0
    assert np.array_equal(tree.view(np.int64), before.view(np.int64))
    assert not st.any()


def host_tree(lib, cap, idx, leaves):
    tree = np.full(4 * cap, np.nan)
    assert lib.smi_per_init_host(_p(tree), cap) == 0
    i, v = np.asarray(idx, dtype=np.int64), np.asarray(leaves, dtype=np.float64)
    assert lib.smi_per_set_host(_p(tree), cap, _p(i), _p(v), len(i)) == 0
    return tree


def test_init_host_matches_per_ref():
    lib = _lib()
    tree = np.full(32, np.nan)
    assert lib.smi_per_init_host(_p(tree), 8) == 0
    assert np.array_equal(tree.view(np.int64), PR.PerRef(8).buffer().view(np.int64))


@pytest.mark.parametrize('case', PR.tree_cases(), ids=lambda c: c[0])
def test_set_host_matches_per_ref(case):
    """the whole tree buffer bit-equal; a repeated slot keeps its last value"""
    _, cap, idx, leaves = case
    ref = PR.PerRef(cap)
    ref.set(idx, leaves)
    tree = host_tree(_lib(), cap, idx, leaves)
    assert np.array_equal(tree.view(np.int64), ref.buffer().view(np.int64))
    last = {s: v for s, v in zip(idx, leaves)}
    for s, v in last.items():
        assert tree[2 * (cap + s)] == v and tree[2 * (cap + s) + 1] == v


def library_stream(lib, advanced):
    """the library's own state after smi_mt_seed(DRAW_SEED), optionally advanced
    by an odd number of words through smi_mt_randint_host"""
    st = np.zeros(625, dtype=np.uint32)
    assert lib.smi_mt_seed(PR.DRAW_SEED, _p(st)) == 0
    if advanced:
        m, n = PR.DRAW_ADVANCE
        tmp = np.zeros(m, dtype=np.int64)
        assert lib.smi_mt_randint_host(_p(st), n, m, _p(tmp)) == 0
        assert int(st[624]) % 2 == 1
    return st


@pytest.mark.parametrize('cap', PR.DRAW_CAPS)
@pytest.mark.parametrize('which', range(4))
def test_sample_host_matches_cpython(cap, which):
    lib = _lib()
    length = PR.draw_lengths(cap)[which]
    leaves = PR.draw_tree(cap, length)
    tree = host_tree(lib, cap, np.arange(length), leaves[:length])
    ref = PR.PerRef.from_leaves(cap, leaves)
    assert np.array_equal(tree.view(np.int64), ref.buffer().view(np.int64))
    for batch in PR.DRAW_BATCHES:
        for advanced in (False, True):
            st = library_stream(lib, advanced)
            assert np.array_equal(st, PR.seed_stream(advanced))     # leaves random.* at that state
            want, w64 = ref.sample(length, batch, 0.4)
            idx = np.full(batch, -1, dtype=np.int64)
            w = np.zeros(batch, dtype=np.float32)
            assert lib.smi_per_sample_host(_p(tree), cap, length, _p(st), batch, 0.4, _p(idx),
                                           _p(w)) == 0
            assert idx.tolist() == want, (cap, length, batch, advanced)
            assert np.array_equal(st, PR.mt_state()), (cap, length, batch, advanced)
            assert length - 1 not in idx.tolist()
            # fp64 pow is orders below one float32 rounding: the stored value is
            # at most one float32 ulp from the truth
            w64 = np.asarray(w64)
            assert np.all(np.abs(w.astype(np.float64) - w64) <= 2.0 ** -23 * w64)


def test_beta_zero_gives_exactly_one():
    lib = _lib()
    cap, length = 1024, 700
    leaves = PR.draw_tree(cap, length)
    tree = host_tree(lib, cap, np.arange(length), leaves[:length])
    st = library_stream(lib, False)
    idx, w = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.float32)
    assert lib.smi_per_sample_host(_p(tree), cap, length, _p(st), 64, 0.0, _p(idx), _p(w)) == 0
    assert np.array_equal(w.view(np.int32), np.ones(64, dtype=np.float32).view(np.int32))


def test_total_leaves_out_the_last_slot():
    """per_ref's recursive reduce against a plain left-to-right statement of
    its association, so the oracle itself is pinned"""
    random.seed(3)
    for cap in (2, 8, 64):
        for length in range(2, cap + 1):
            leaves = PR.draw_tree(cap, length)
            ref = PR.PerRef.from_leaves(cap, leaves)
            got = ref.total(length)
            assert abs(got - float(np.sum(leaves[:length - 1]))) <= 1e-12 * got
