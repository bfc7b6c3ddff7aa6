"""Test-side restatement of the prioritized replay's trees, draw, weights and
priority updates (surreal_amd/csrc/per_kernels.hip, decisions 1-5 of its
header) over plain Python floats.  It is the openai/baselines segment-tree
arithmetic written out from those rules: recursive reduce, iterative
find_prefixsum_idx, random.random() of the live interpreter."""
import math
import random

import numpy as np


def capacity_for(memory_size):
    cap = 1
    while cap < memory_size:
        cap *= 2
    return cap


class PerRef(object):
    def __init__(self, cap):
        assert cap >= 1 and cap & (cap - 1) == 0
        self.cap = cap
        self.sum = [0.0] * (2 * cap)
        self.min = [math.inf] * (2 * cap)
        self.max_priority = 1.0

    # ------------------------------------------------------------- trees
    def set_leaf(self, slot, value):
        """segment_tree.__setitem__: the leaf, then every parent from its two
        children"""
        i = self.cap + slot
        self.sum[i] = value
        self.min[i] = value
        i //= 2
        while i >= 1:
            self.sum[i] = self.sum[2 * i] + self.sum[2 * i + 1]
            self.min[i] = min(self.min[2 * i], self.min[2 * i + 1])
            i //= 2

    def set(self, idx, leaves):
        for s, v in zip(idx, leaves):           # the sequential loop: the last one stands
            self.set_leaf(int(s), float(v))

    def _reduce(self, start, end, node, node_start, node_end):
        if start == node_start and end == node_end:
            return self.sum[node]
        mid = (node_start + node_end) // 2
        if end <= mid:
            return self._reduce(start, end, 2 * node, node_start, mid)
        if mid + 1 <= start:
            return self._reduce(start, end, 2 * node + 1, mid + 1, node_end)
        return (self._reduce(start, mid, 2 * node, node_start, mid) +
                self._reduce(mid + 1, end, 2 * node + 1, mid + 1, node_end))

    def sum_range(self, start, end):
        """segment_tree.sum(start, end): reduce subtracts one from `end`"""
        end -= 1
        return self._reduce(start, end, 1, 0, self.cap - 1)

    def total(self, length):
        return self.sum_range(0, length - 1)    # slots 0 .. length-2

    def find_prefixsum_idx(self, mass):
        i = 1
        while i < self.cap:
            if self.sum[2 * i] > mass:
                i = 2 * i
            else:
                mass -= self.sum[2 * i]
                i = 2 * i + 1
        return i - self.cap

    # ------------------------------------------------------- insert / update
    def insert(self, first_slot, n, memory_size, alpha):
        for j in range(n):                      # one leaf per written row, in ring order
            self.set_leaf((first_slot + j) % memory_size, self.max_priority ** alpha)

    def update_priorities(self, idx, priorities, alpha):
        for s, p in zip(idx, priorities):
            p = float(p)
            assert p > 0
            self.set_leaf(int(s), p ** alpha)
            self.max_priority = max(self.max_priority, p)

    def update_from_td(self, idx, td, eps, alpha):
        self.update_priorities(idx, [abs(float(t)) + eps for t in td], alpha)

    # ------------------------------------------------------------------ draw
    def sample(self, length, batch, beta, rng=random):
        """(indices, fp64 weights); draws from `rng` (the random module after
        random.seed(s), or a random.Random)"""
        assert length >= 2
        total = self.total(length)
        idx = []
        for _ in range(batch):
            mass = rng.random() * total
            idx.append(min(self.find_prefixsum_idx(mass), length - 1))
        return idx, self.weights(idx, length, beta)

    def weights(self, idx, length, beta):
        s = self.sum[1]
        p_min = self.min[1] / s
        max_w = (p_min * length) ** (-beta)
        return [(self.sum[self.cap + i] / s * length) ** (-beta) / max_w for i in idx]

    # ---------------------------------------------------------------- buffer
    def buffer(self):
        """the library's layout: node i = {sum, min} at [2i], [2i+1]; [0] =
        max_priority, [1] = 0.0"""
        out = np.zeros(4 * self.cap, dtype=np.float64)
        out[0::2] = self.sum
        out[1::2] = self.min
        out[0], out[1] = self.max_priority, 0.0
        return out

    @classmethod
    def from_leaves(cls, cap, leaves, max_priority=1.0):
        """a tree whose sum leaves are `leaves` (min leaf = sum leaf where it is
        non-zero, +inf where the slot is empty) and every ancestor recomputed"""
        t = cls(cap)
        for s, v in enumerate(leaves):
            v = float(v)
            t.sum[cap + s] = v
            t.min[cap + s] = v if v != 0.0 else math.inf
        for i in range(cap - 1, 0, -1):
            t.sum[i] = t.sum[2 * i] + t.sum[2 * i + 1]
            t.min[i] = min(t.min[2 * i], t.min[2 * i + 1])
        t.max_priority = max_priority
        return t


def mt_state():
    """the live interpreter's MT19937 state as the library's 625 words"""
    return np.array(random.getstate()[1], dtype=np.uint32)


def spread_leaves(n, seed):
    """n leaves spanning 1e-6 .. 1e3 (log-uniform)"""
    r = np.random.RandomState(seed)
    return 10.0 ** r.uniform(-6.0, 3.0, size=n)


# ------------------------------------------------- cases shared by the tests
def tree_cases():
    """(name, cap, idx, leaves): cap 2, cap 8, and cap 256 with 37 indices that
    include one slot three times with three values and both end slots"""
    r = np.random.RandomState(5)
    others = r.choice([i for i in range(1, 255) if i != 77], size=32, replace=False).tolist()
    idx256 = [0, 255] + others[:10] + [77] + others[10:20] + [77] + others[20:] + [77]
    assert len(idx256) == 37 and idx256.count(77) == 3 and len(set(idx256)) == 35
    return [('cap2', 2, [1, 0], [2.0, 0.5]),
            ('cap8', 8, [3, 0, 7, 5], [0.25, 1.5, 3.0, 1e-3]),
            ('cap256', 256, idx256, spread_leaves(37, 6).tolist())]


DRAW_CAPS = (8, 1024)
DRAW_BATCHES = (1, 37, 400)                     # 400 draws = 800 words: more than one twist
DRAW_SEED = 12345
DRAW_ADVANCE = (3, 7)                           # randint(0, 6) x 3 before the draw: an odd word count


def draw_lengths(cap):
    return (2, 3, cap // 2 + 1, cap)


def draw_tree(cap, length):
    """leaves 1e-6 .. 1e3 on slots 0 .. length-1, the rest empty"""
    leaves = np.zeros(cap)
    leaves[:length] = spread_leaves(length, 100 + cap + length)
    return leaves


def seed_stream(advanced):
    """random.seed(DRAW_SEED), optionally advanced by an odd number of words;
    returns the live state as the library's 625 words"""
    random.seed(DRAW_SEED)
    if advanced:
        m, n = DRAW_ADVANCE
        for _ in range(m):
            random.randint(0, n - 1)
    return mt_state()


def ref_from_device(tree, cap):
    """per_ref tree rebuilt from the device's own leaves (every ancestor
    recomputed in Python) and max_priority"""
    t = tree.cpu().numpy()
    return PerRef.from_leaves(cap, t[2 * cap::2], max_priority=float(t[0])), t


def check_drawn_leaves(tree, cap, want, td):
    """the leaves of the drawn slots are (|td| + 1e-6) ** 0.6 (a repeated slot
    keeps its last) to 2 ulp = 2^-51 relative: the device's fp64 pow against
    the host's (test_gpu_dqn.py::test_prioritized_replay_loop)"""
    leaves = tree.cpu().numpy()[2 * cap::2]
    last = {s: (abs(float(v)) + 1e-6) ** 0.6 for s, v in zip(want, td)}
    slots = np.array(sorted(last))
    exp = np.array([last[s] for s in slots])
    rel = np.abs(leaves[slots] - exp) / exp
    print('leaf max relative difference from the host pow:', rel.max())
    assert (rel <= 2.0 ** -51).all()
