"""CPU tests of the frame-shared pixel replay: the host allocator
(surreal_amd/frame_store.py) against a brute-force model, its rollback when the
store is full, the accepted camera forms, and the argument checks of
smi_replay_gather_shared / smi_replay_insert_shared (no launch is made)."""
import ctypes
import random

import numpy as np
import pytest

S = 3
CHUNKS = (1, 3, 18, 9, 1, 3, 18, 9)         # 62 transitions into 7 slots: 8 wraps


def rolling_stream(n_step, total, frame_shape=(1, 4, 4), seed=0, actors=2):
    """`total` transitions of `actors` interleaved actors as (obs frames,
    obs_next frames), each a list of S uint8 arrays.  Episodes last 1..9 steps
    and start from a reset observation whose S frames are one frame; every step
    appends one new frame; obs_next is n_step steps after obs and an episode's
    last n_step - 1 steps send nothing (ExpSenderWrapperSSARNStepBootstrap,
    env/exp_sender_wrapper.py:95-112).  Frames an actor's observations share
    are the same array objects, as in the reference sender."""
    rs = np.random.RandomState(seed)
    rnd = random.Random(seed)

    def frame():
        return rs.randint(0, 256, frame_shape).astype(np.uint8)

    def episodes():
        while True:
            steps = rnd.randint(1, 9)
            hist = [frame()] * S                   # the reset observation
            obs = [list(hist)]
            for _ in range(steps):
                hist = hist[1:] + [frame()]
                obs.append(list(hist))
                if len(obs) > n_step:
                    yield obs[-1 - n_step], obs[-1]
                else:
                    yield None
    gens = [episodes() for _ in range(actors)]
    out = []
    while len(out) < total:
        for g in gens:
            t = next(g)
            if t is not None and len(out) < total:
                out.append(t)
    return out


def _bytes(frames):
    return tuple(f.tobytes() for f in frames)


class Model(object):
    """the ring as plain Python: slot -> the two observations' frame bytes"""

    def __init__(self, memory_size):
        self.ring = [None] * memory_size
        self.next = 0

    def insert(self, transitions):
        for o0, o1 in transitions:
            self.ring[self.next] = (_bytes(o0), _bytes(o1))
            self.next = (self.next + 1) % len(self.ring)

    def live(self):
        return [(i, t) for i, t in enumerate(self.ring) if t is not None]

    def distinct(self):
        return len({f for _, t in self.live() for side in t for f in side})


def _insert(alloc, store, chunk):
    """insert a chunk as UniformReplay does and keep the store's bytes"""
    skip = max(0, len(chunk) - alloc.memory_size)
    first, ids, fslots, new = alloc.insert(chunk[skip:], skipped=skip)
    assert len(set(fslots.tolist())) == len(fslots) == len(new)     # one write per slot and call
    assert ids.shape == (len(chunk) - skip, 2, S) and ids.dtype == np.int32
    for s, f in zip(fslots.tolist(), new):
        store[s] = f.tobytes()
    return first, ids, fslots


def _check(alloc, store, model):
    live = model.live()
    assert len(alloc) == len(live)
    assert alloc.frames_in_use == model.distinct()
    assert int((alloc.refcount > 0).sum()) == alloc.frames_in_use
    assert int(alloc.refcount.sum()) == 2 * S * len(live)
    assert alloc.refcount.min() >= 0
    for slot, t in live:
        for side in range(2):
            got = tuple(store[int(s)] for s in alloc.ids[slot, side])
            assert got == t[side], (slot, side)
    # every live key has a slot of its own, and free slots are exactly the unreferenced ones
    assert len(set(alloc.slot_of.values())) == len(alloc.slot_of) == alloc.frames_in_use
    assert sorted(alloc.free) == [s for s in range(alloc.frame_slots) if alloc.refcount[s] == 0]


@pytest.mark.parametrize('n_step', [1, 3])
def test_allocator_matches_brute_force_model(n_step):
    from surreal_amd.frame_store import FrameAllocator
    M = 7
    stream = rolling_stream(n_step, sum(CHUNKS), seed=n_step)
    alloc, store, model = FrameAllocator(M, M + M // 4 + 2 * S * 4, S), {}, Model(M)
    pos = 0
    for n in CHUNKS:
        chunk = stream[pos:pos + n]
        pos += n
        first, ids, _ = _insert(alloc, store, chunk)
        model.insert(chunk)
        assert alloc._next_idx == model.next == pos % M
        assert first == (pos - min(n, M)) % M
        assert np.array_equal(alloc.ids[(first + np.arange(len(ids))) % M], ids)
        _check(alloc, store, model)
    assert pos >= 5 * M
    # consecutive transitions share frames: far fewer than 2 S per transition
    assert alloc.frames_in_use < 2 * S * len(alloc)


@pytest.mark.parametrize('n_step', [1, 3])
def test_bulk_insert_equals_single_inserts(n_step):
    from surreal_amd.frame_store import FrameAllocator
    M = 7
    stream = rolling_stream(n_step, sum(CHUNKS), seed=10 + n_step)
    bulk, one = FrameAllocator(M, 40, S), FrameAllocator(M, 40, S)
    sb, so = {}, {}
    pos = 0
    for n in CHUNKS:
        chunk = stream[pos:pos + n]
        pos += n
        _insert(bulk, sb, chunk)
        for t in chunk:
            _insert(one, so, [t])
        assert len(bulk) == len(one) and bulk._next_idx == one._next_idx
        assert bulk.frames_in_use == one.frames_in_use
        for slot in range(len(bulk)):
            for side in range(2):
                assert [sb[int(s)] for s in bulk.ids[slot, side]] == \
                    [so[int(s)] for s in one.ids[slot, side]]


def test_identity_is_hashed_once_and_digest_finds_copies(monkeypatch):
    from surreal_amd import frame_store
    calls = []
    real = frame_store.frame_digest

    def counting(f):
        calls.append(id(f))
        return real(f)
    monkeypatch.setattr(frame_store, 'frame_digest', counting)
    rs = np.random.RandomState(3)
    f = [rs.randint(0, 256, (1, 4, 4)).astype(np.uint8) for _ in range(5)]
    # three experiences of one actor: f[0..2] -> f[1..3] -> f[2..4], objects shared
    chunk = [(f[0:3], f[1:4]), (f[1:4], f[2:5]), (f[2:5], f[2:5])]
    alloc = frame_store.FrameAllocator(7, 16, S)
    _, _, fslots, new = alloc.insert(chunk)
    assert len(calls) == 5 and len(set(calls)) == 5         # 18 references, 5 objects
    assert len(fslots) == 5 and alloc.frames_in_use == 5
    assert [n.tobytes() for n in new] == [x.tobytes() for x in f]
    # a later call: identity is gone, equal-content copies are found by digest
    del calls[:]
    copies = [x.copy() for x in f]
    _, ids, fslots, _ = alloc.insert([(copies[0:3], copies[2:5])])
    assert len(calls) == 5 and len(fslots) == 0 and alloc.frames_in_use == 5
    assert ids[0, 0].tolist() == alloc.ids[0, 0].tolist()
    assert ids[0, 1].tolist() == alloc.ids[2, 0].tolist()


def _state(a):
    return (a.refcount.tobytes(), list(a.free), dict(a.slot_of), list(a.key_of), a.ids.tobytes(),
            a._len, a._next_idx)


def _distinct(n, seed):
    rs = np.random.RandomState(seed)
    return [([rs.randint(0, 256, (1, 4, 4)).astype(np.uint8) for _ in range(S)],
             [rs.randint(0, 256, (1, 4, 4)).astype(np.uint8) for _ in range(S)])
            for _ in range(n)]


def test_store_full_rolls_back():
    from surreal_amd.frame_store import FrameAllocator
    M = 3
    alloc, store, model = FrameAllocator(M, 16, S), {}, Model(M)
    head = rolling_stream(1, 5, seed=4)
    _insert(alloc, store, head)                     # wraps: the ring is full, frames shared
    model.insert(head)
    _check(alloc, store, model)
    free_before = len(alloc.free)
    assert 6 < free_before < 12                     # the first new transition fits, the second not
    before = _state(alloc)
    with pytest.raises(RuntimeError, match='frame_slots'):
        alloc.insert(_distinct(3, seed=5))          # 18 new frames: fails after a release
    assert _state(alloc) == before
    _check(alloc, store, model)
    # one that fits goes in, and the bookkeeping still matches the model
    one = _distinct(1, seed=6)
    _insert(alloc, store, one)
    model.insert(one)
    _check(alloc, store, model)
    # an all-distinct stream into a store too small for a ring of them
    small = FrameAllocator(7, 20, S)
    small.insert(_distinct(3, seed=7))
    before = _state(small)
    with pytest.raises(RuntimeError, match='frame_slots'):
        small.insert(_distinct(1, seed=8))
    assert _state(small) == before


def test_camera_forms_give_the_same_keys():
    from surreal_amd.frame_store import frame_digest, split_camera
    rs = np.random.RandomState(9)
    cam = rs.randint(0, 256, (9, 5, 4)).astype(np.uint8)
    shape = (3, 5, 4)
    whole = split_camera(cam, S, shape)
    as_list = split_camera([cam[0:3], cam[3:6], cam[6:9]], S, shape)
    as_float = split_camera(cam.astype(np.float64), S, shape)
    keys = [frame_digest(f) for f in whole]
    assert len(set(keys)) == S
    assert [frame_digest(f) for f in as_list] == keys
    assert [frame_digest(f) for f in as_float] == keys
    for f in whole + as_list + as_float:
        assert f.dtype == np.uint8 and f.shape == shape and f.flags['C_CONTIGUOUS']
    # one object named twice in a call comes back as the same frames
    cache = {}
    assert split_camera(cam, S, shape, cache)[0] is split_camera(cam, S, shape, cache)[0]
    # the dtype and range rules of _camera_u8
    for v in (0.5, -1.0, 256.0):
        with pytest.raises(TypeError):
            split_camera(np.full((9, 5, 4), v), S, shape)
        with pytest.raises(TypeError):
            split_camera([cam[0:3], np.full(shape, v), cam[6:9]], S, shape)
    with pytest.raises(ValueError):
        split_camera(cam[:, :4], S, shape)
    with pytest.raises(ValueError):
        split_camera([cam[0:3], cam[3:6], cam[6:8]], S, shape)


def test_share_frames_config_errors():
    import copy
    from surreal_amd.config import DDPG_DEFAULT_LEARNER_CONFIG, gym_env_config, pixel_env_config
    from surreal_amd.frame_store import frame_sharing
    lc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
    lc.replay.memory_size = 333333
    ec = pixel_env_config(17, 6, (9, 84, 84))
    ec['frame_stacks'] = 3
    assert frame_sharing(lc, ec) is None            # the option is off by default
    lc.replay.share_frames = False
    assert frame_sharing(lc, ec) is None
    lc.replay.share_frames = True
    assert frame_sharing(lc, ec) == (3, (3, 84, 84), 416666)
    lc.replay.frame_slots = 1000
    assert frame_sharing(lc, ec) == (3, (3, 84, 84), 1000)
    ec['frame_stacks'] = 2                          # 9 % 2 != 0
    with pytest.raises(ValueError, match='frame_stacks'):
        frame_sharing(lc, ec)
    with pytest.raises(ValueError, match='pixel'):
        frame_sharing(lc, gym_env_config(17, 6))


def test_replay_gather_shared_rejects_bad_args():
    from surreal_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)                  # never dereferenced: no launch is made

    def bad(*args):
        assert lib.smi_replay_gather_shared(*args) == -1
        assert b'replay_gather_shared' in lib.smi_last_error()

    #   table cols store fid S fbytes idx batch rows pix pixn stream
    bad(None, 0, None, p, 3, 1200, p, 4, None, p, p, None)             # NULL store
    bad(None, 0, p, None, 3, 1200, p, 4, None, p, p, None)             # NULL ids
    bad(None, 0, p, p, 3, 1200, None, 4, None, p, p, None)             # NULL idx
    bad(None, 0, p, p, 3, 1200, p, 4, None, None, p, None)             # NULL pix_out
    bad(None, 0, p, p, 3, 1200, p, 4, None, p, None, None)             # NULL pix_next_out
    bad(None, 0, p, p, 0, 1200, p, 4, None, p, p, None)                # stack = 0
    bad(None, 0, p, p, 5, 1200, p, 4, None, p, p, None)                # stack = 5
    bad(None, 0, p, p, 3, 0, p, 4, None, p, p, None)                   # fbytes = 0
    bad(None, 0, p, p, 3, (1 << 31) // 3, p, 4, None, p, p, None)      # S * fbytes reaches 2^31
    bad(None, 0, p, p, 1, 1 << 31, p, 4, None, p, p, None)
    bad(None, 0, p, p, 3, 1200, p, -1, None, p, p, None)               # batch = -1
    bad(None, -1, p, p, 3, 1200, p, 4, None, p, p, None)               # cols = -1
    bad(None, 4, p, p, 3, 1200, p, 4, p, p, p, None)                   # cols = 4, NULL table
    bad(p, 4, p, p, 3, 1200, p, 4, None, p, p, None)                   # cols = 4, NULL rows_out
    assert lib.smi_replay_gather_shared(p, 4, p, p, 3, 1200, p, 0, p, p, p, None) == 0   # batch = 0
    assert lib.smi_replay_gather_shared(None, 0, p, p, 4, (1 << 31) // 4 - 1, p, 0, None, p, p,
                                        None) == 0


def test_replay_insert_shared_rejects_bad_args():
    from surreal_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)

    def bad(*args):
        assert lib.smi_replay_insert_shared(*args) == -1
        assert b'replay_insert_shared' in lib.smi_last_error()

    #   table cols fid S store fbytes mem first rows ids n frames fslots m stream
    bad(p, 4, None, 3, p, 1200, 7, 0, p, p, 2, p, p, 1, None)          # NULL ids ring
    bad(p, 4, p, 3, None, 1200, 7, 0, p, p, 2, p, p, 1, None)          # NULL store
    bad(p, 4, p, 0, p, 1200, 7, 0, p, p, 2, p, p, 1, None)             # stack = 0
    bad(p, 4, p, 5, p, 1200, 7, 0, p, p, 2, p, p, 1, None)             # stack = 5
    bad(p, 4, p, 3, p, 0, 7, 0, p, p, 2, p, p, 1, None)                # fbytes = 0
    bad(p, 4, p, 3, p, (1 << 31) // 3, 7, 0, p, p, 2, p, p, 1, None)   # fbytes too large
    bad(p, 4, p, 3, p, 1200, 7, 0, p, p, -1, p, p, 1, None)            # n = -1
    bad(p, 4, p, 3, p, 1200, 7, 0, p, p, 2, p, p, -1, None)            # m = -1
    bad(p, -1, p, 3, p, 1200, 7, 0, p, p, 2, p, p, 1, None)            # cols = -1
    bad(p, 4, p, 3, p, 1200, 0, 0, p, p, 2, p, p, 1, None)             # memory_size = 0
    bad(p, 4, p, 3, p, 1200, 7, 7, p, p, 2, p, p, 1, None)             # first_slot = memory_size
    bad(p, 4, p, 3, p, 1200, 7, -1, p, p, 2, p, p, 1, None)            # first_slot = -1
    bad(p, 4, p, 3, p, 1200, 7, 0, p, None, 2, p, p, 1, None)          # n > 0, NULL ids
    bad(p, 4, p, 3, p, 1200, 7, 0, None, p, 2, p, p, 1, None)          # n > 0, cols > 0, NULL rows
    bad(None, 4, p, 3, p, 1200, 7, 0, p, p, 2, p, p, 1, None)          # n > 0, cols > 0, NULL table
    bad(p, 4, p, 3, p, 1200, 7, 0, p, p, 2, None, p, 1, None)          # m > 0, NULL frames
    bad(p, 4, p, 3, p, 1200, 7, 0, p, p, 2, p, None, 1, None)          # m > 0, NULL fslots
    assert lib.smi_replay_insert_shared(p, 4, p, 3, p, 1200, 7, 0, p, p, 0, p, p, 0, None) == 0
    assert lib.smi_replay_insert_shared(None, 0, p, 3, p, 1200, 7, 6, None, None, 0, None, None, 0,
                                        None) == 0
